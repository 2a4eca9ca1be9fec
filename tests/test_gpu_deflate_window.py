"""GPU: device deflate at deflateInit2's windowBits 9..14 (the zng_rocm_*_window_* calls; lz_rows_win_kernel, the window form
of the rows matcher), black-box.  The oracle is independent of the code under test: tests/deflate_parse.py takes every output
apart into tokens, tests/window_cases.py plants the repeats and measures the coverage (tests/test_window_cases_cpu.py holds
CPython's zlib to the same cells at the same window), and CPython's zlib stands in for a reader that really has a 1 << w
window: decompressobj(-w) fed 97 output bytes at a time, so that copies go through its window.

  cap        at every level 1..9 no token of any stream has a distance above cap = (1 << w) - 262, none reaches in front of
             history + stream, and every range whose only copy lies cap + 1, 1 << w or 32506 back is literals throughout
  recall     at every level each judged range (two where the 131072 segment border cuts it) has at most 3 literal bytes and
             every overlapping match has distance D (far form) or a multiple of D (near form) -- the rule of test_rows_recall --
             the cells whose source lies exactly cap in front of a segment's first byte (priming) included
             (not asked where CPython's zlib itself does not show it: window_cases.cpython_misses, w 9 at level 1 only)
  15         the four new calls with window_bits = 15 give the bytes of the existing four
  reader     the six classes of synth.segment through the chunked small-window reader, raw, zlib and gzip; the zlib header is
             CPython's, and a reader opened one window smaller answers "invalid window size"
  size       device size / CPython size at the same level and wbits stays within 0.01 of the ratio measured when this file was
             written (SIZE_RATIO)
  strategies, function of the input, the members file, the refusals, the bound"""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import deflate_parse as dp
import matcher_cases as mc
import synth
import window_cases as wc
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu

LEVELS = tuple(range(1, 10))
EINVAL = -3
CANARY = 0xA5

# device size / CPython zlib size (raw deflate, the same level and wbits), 256 KiB of each class of synth.segment
# (_size_classes); measured on MI355X.  The output is deterministic: the 0.01 the test adds is room for later changes, not noise.
# Keys are "window-level"; the same measure at 15 is test_gpu_matcher_recall.py's SIZE_RATIO (rows-1, rows-6, rows-9).
SIZE_SEED = 0x5123
SIZE_RATIO = {
    "9-1": {"text": 0.9890, "records": 1.0258, "dna": 0.9195, "sparse": 0.7318, "random": 0.9980, "xml": 0.9856},
    "9-6": {"text": 1.0305, "records": 1.1909, "dna": 0.9511, "sparse": 0.8817, "random": 0.9980, "xml": 1.0187},
    "9-9": {"text": 1.0305, "records": 1.1909, "dna": 0.9511, "sparse": 1.0561, "random": 0.9980, "xml": 1.0187},
    "10-1": {"text": 0.9490, "records": 1.0265, "dna": 0.9518, "sparse": 0.7092, "random": 0.9980, "xml": 0.9681},
    "10-6": {"text": 1.0048, "records": 1.1151, "dna": 0.9673, "sparse": 0.8733, "random": 0.9980, "xml": 0.9957},
    "10-9": {"text": 1.0049, "records": 1.1156, "dna": 0.9673, "sparse": 0.9783, "random": 0.9980, "xml": 0.9957},
    "11-1": {"text": 0.9334, "records": 1.0470, "dna": 0.9890, "sparse": 0.7091, "random": 0.9980, "xml": 0.9675},
    "11-6": {"text": 0.9975, "records": 1.0592, "dna": 0.9713, "sparse": 0.8723, "random": 0.9980, "xml": 0.9916},
    "11-9": {"text": 0.9979, "records": 1.0604, "dna": 0.9713, "sparse": 0.9693, "random": 0.9980, "xml": 0.9916},
    "12-1": {"text": 0.9236, "records": 1.0497, "dna": 0.9887, "sparse": 0.7063, "random": 0.9979, "xml": 0.9636},
    "12-6": {"text": 0.9959, "records": 1.0351, "dna": 0.9830, "sparse": 0.8691, "random": 0.9979, "xml": 0.9966},
    "12-9": {"text": 1.0002, "records": 1.0349, "dna": 0.9831, "sparse": 0.9721, "random": 0.9979, "xml": 0.9966},
    "13-1": {"text": 0.9162, "records": 1.0473, "dna": 0.9893, "sparse": 0.6996, "random": 0.9979, "xml": 0.9562},
    "13-6": {"text": 1.0018, "records": 1.0152, "dna": 0.9969, "sparse": 0.8650, "random": 0.9979, "xml": 0.9969},
    "13-9": {"text": 1.0126, "records": 1.0124, "dna": 0.9976, "sparse": 0.9744, "random": 0.9979, "xml": 0.9972},
    "14-1": {"text": 0.9093, "records": 1.0474, "dna": 0.9888, "sparse": 0.6916, "random": 0.9998, "xml": 0.9541},
    "14-6": {"text": 1.0068, "records": 0.9991, "dna": 0.9926, "sparse": 0.8642, "random": 0.9998, "xml": 1.0018},
    "14-9": {"text": 1.0238, "records": 0.9950, "dna": 1.0002, "sparse": 0.9744, "random": 0.9998, "xml": 1.0103},
}


class Device:
    def __init__(self):
        zr = product()
        zr.init()
        self.torch = torch_mod()
        self.dfl = importlib.import_module("zlib-ng_amd.deflate")
        self.inf = importlib.import_module("zlib-ng_amd.inflate")
        self.rocm = importlib.import_module("zlib-ng_amd.rocm")
        self.lib = self.rocm.lib()
        self._packed, self._judged = {}, {}

    def packed(self, w):
        """the cells of window w in one host buffer, on the device"""
        if w not in self._packed:
            cells = wc.cells(w)
            host, offs, lens, dls = mc.pack([(c.history, c.data) for c in cells])
            assert host.size < 32 << 20                        # one call of this size cuts 128 KiB segments
            self._packed[w] = (cells, self.torch.from_numpy(host).cuda(), offs, lens, dls)
        return self._packed[w]

    def batch(self, streams, level, w, strategy=0, histories=None):
        """[compressed bytes] of `streams` through one StreamsBatch call"""
        items = [(histories[i] if histories else b"", s) for i, s in enumerate(streams)]
        host, offs, lens, dls = mc.pack(items)
        b = self.dfl.StreamsBatch(self.torch.from_numpy(host).cuda(), offs, lens, dict_len=dls)
        b.run(level=level, strategy=strategy, window_bits=w)
        return [b.compressed(i) for i in range(b.n)]

    def judged(self, w, level):
        """(cap misses, recall misses, worst cell) of all cells of window w at `level`: ONE StreamsBatch call, every stream
        parsed once"""
        if (w, level) not in self._judged:
            cells, src, offs, lens, dls = self.packed(w)
            b = self.dfl.StreamsBatch(src, offs, lens, dict_len=dls)
            b.run(level=level, window_bits=w)
            whole = b.dst.cpu().numpy()
            cap_bad, recall_bad, worst = [], [], (0, "")
            for i, c in enumerate(cells):
                comp = whole[b.out_off[i]:b.out_off[i] + int(b.out_lens[i])].tobytes()
                p = dp.parse(comp, history=c.history)
                assert p.data == c.data, c.name
                assert (p.end_bit + 7) // 8 == len(comp), c.name
                wrong = wc.limits(c, p)
                if wrong:
                    cap_bad.append((c.name, wrong))
                if not c.too_far and not wc.cpython_misses(c, level):
                    got, ok = wc.recall(c, p)
                    worst = max(worst, (max(g[0] for g in got), c.name))
                    if not ok:
                        recall_bad.append((c.name, got))
            self._judged[w, level] = (cap_bad, recall_bad, worst)
        return self._judged[w, level]


@pytest.fixture(scope="module")
def dev():
    return Device()


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("w", wc.WINDOWS)
def test_cap(dev, w, level):
    cap_bad, _, _ = dev.judged(w, level)
    assert not cap_bad, cap_bad


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("w", wc.WINDOWS)
def test_recall(dev, w, level):
    _, recall_bad, worst = dev.judged(w, level)
    print("window %d level %d: worst cell %s with %d literal bytes; %d cells miss" % (w, level, worst[1], worst[0], len(recall_bad)))
    for b in recall_bad:
        print("  MISS", b)
    assert not recall_bad, recall_bad


# ---- the same bytes at 15 ---------------------------------------------------------------------------------------------------
def _fifteen_inputs():
    pos = [c.data for c in mc.cells() if c.sweep == "pos"]
    return pos + [synth.silesia_like(300 << 10, seed=0xD37).tobytes()]


def _streams_call(dev, b, level, strategy, w):
    """zng_rocm_deflate_window_streams_dev (w given) or zng_rocm_deflate_strategy_streams_dev over the batch b, outputs zeroed
    first: (status, lengths, the whole output tensor)"""
    b.dst.zero_()
    for i in range(b.n):
        b.out_lens[i] = 0
    st = dev.rocm._stream_ptr(None)
    if w is None:
        rc = dev.lib.zng_rocm_deflate_strategy_streams_dev(level, strategy, C.byref(b.jobs), b.n, C.byref(b.out_lens), st)
    else:
        rc = dev.lib.zng_rocm_deflate_window_streams_dev(level, strategy, w, C.byref(b.jobs), b.n, C.byref(b.out_lens), st)
    dev.torch.cuda.synchronize()
    return rc, [int(v) for v in b.out_lens], b.dst.clone()


def _block_call(dev, src, off, n, level, strategy, w):
    cap = dev.dfl.deflate_bound(n)
    dst = dev.torch.zeros(cap, dtype=dev.torch.uint8, device="cuda")
    out_len = C.c_size_t(0)
    st = dev.rocm._stream_ptr(None)
    if w is None:
        rc = dev.lib.zng_rocm_deflate_strategy_block_dev(level, strategy, dev.rocm._dev_ptr(src, off), n, 0, 0, dev.rocm._dev_ptr(dst), cap,
                                                         C.byref(out_len), st)
    else:
        rc = dev.lib.zng_rocm_deflate_window_block_dev(level, strategy, w, dev.rocm._dev_ptr(src, off), n, 0, 0, dev.rocm._dev_ptr(dst),
                                                       cap, C.byref(out_len), st)
    return rc, int(out_len.value), dst


class Wrapped:
    """the job table of the wrapped pair over views of one source tensor, every member buffer and result word behind a canary"""

    def __init__(self, dev, src, offs, lens, fmt):
        torch, dfl = dev.torch, dev.dfl
        self.n, self.fmt = len(lens), fmt
        self.bounds = [(dfl.compress_streams2_bound(n, fmt) + 15) & ~15 for n in lens]
        self.out_off = np.concatenate([[0], np.cumsum(self.bounds)]).tolist()
        self.dst = torch.full((self.out_off[-1],), CANARY, dtype=torch.uint8, device="cuda")
        self.results = torch.full((self.n, 2), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
        self.offsets = torch.full((self.n + 1,), -0x5A5A5A5B, dtype=torch.int64, device="cuda")
        self.checks = torch.full((self.n,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
        self.whole = torch.full((self.out_off[-1],), CANARY, dtype=torch.uint8, device="cuda")
        self.srcs = [src[o:o + n] for o, n in zip(offs, lens)]
        self.jobs = dfl.stream_jobs(self.srcs, [self.dst[self.out_off[i]:self.out_off[i] + self.bounds[i]] for i in range(self.n)])

    def reset(self):
        self.dst.fill_(CANARY)
        self.whole.fill_(CANARY)
        self.results.fill_(-0x5A5A5A5B)
        self.offsets.fill_(-0x5A5A5A5B)
        self.checks.fill_(-0x5A5A5A5B)

    def untouched(self):
        return bool((self.dst == CANARY).all()) and bool((self.whole == CANARY).all()) and bool((self.results == -0x5A5A5A5B).all()) \
            and bool((self.offsets == -0x5A5A5A5B).all()) and bool((self.checks == -0x5A5A5A5B).all())

    def streams2(self, dev, level, strategy, w):
        """(status, result words, the member buffers): zng_rocm_compress_streams2_window_dev, or without w the call it extends"""
        self.reset()
        st = dev.rocm._stream_ptr(None)
        if w is None:
            rc = dev.lib.zng_rocm_compress_streams2_dev(self.fmt, level, strategy, C.byref(self.jobs), self.n, 0,
                                                        dev.rocm._dev_ptr(self.results), st)
        else:
            rc = dev.lib.zng_rocm_compress_streams2_window_dev(self.fmt, level, strategy, w, C.byref(self.jobs), self.n, 0,
                                                               dev.rocm._dev_ptr(self.results), st)
        dev.torch.cuda.synchronize()
        return rc, self.results.clone(), self.dst.clone()

    def members(self, dev, level, strategy, w):
        self.reset()
        st = dev.rocm._stream_ptr(None)
        args = (C.byref(self.jobs), self.n, dev.rocm._dev_ptr(self.whole), int(self.whole.numel()), 0, dev.rocm._dev_ptr(self.offsets),
                dev.rocm._dev_ptr(self.checks), st)
        if w is None:
            rc = dev.lib.zng_rocm_compress_members_dev(self.fmt, level, strategy, *args)
        else:
            rc = dev.lib.zng_rocm_compress_members_window_dev(self.fmt, level, strategy, w, *args)
        dev.torch.cuda.synchronize()
        return rc, self.offsets.clone(), self.checks.clone(), self.whole.clone()

    def member(self, res, dst, i):
        return dst[self.out_off[i]:self.out_off[i] + int(res[i, 0])].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def fifteen(dev):
    streams = _fifteen_inputs()
    host, offs, lens, _ = mc.pack([(b"", s) for s in streams])
    assert host.size < 32 << 20
    src = dev.torch.from_numpy(host).cuda()
    return streams, src, offs, lens


@pytest.mark.parametrize("level", (0, 1, 6, 9))
def test_same_bytes_at_15_raw_calls(dev, fifteen, level):
    """zng_rocm_deflate_window_streams_dev and _block_dev at 15 against the strategy calls, strategies 0..4.  (The batch call has
    no level 0: both refuse it alike.)"""
    torch = dev.torch
    streams, src, offs, lens = fifteen
    b = dev.dfl.StreamsBatch(src, offs, lens)
    for strategy in range(5):
        old = _streams_call(dev, b, level, strategy, None)
        new = _streams_call(dev, b, level, strategy, 15)
        assert old[0] == new[0] == (EINVAL if level == 0 else 0), (strategy, old[0], new[0])
        assert old[1] == new[1] and torch.equal(old[2], new[2]), strategy
        assert level == 0 or all(old[1]), strategy
        for i in (0, len(streams) // 2, len(streams) - 1):                       # the single-stream call: three of them
            o = _block_call(dev, src, offs[i], lens[i], level, strategy, None)
            n = _block_call(dev, src, offs[i], lens[i], level, strategy, 15)
            assert o[0] == n[0] == 0 and o[1] == n[1] > 0 and torch.equal(o[2], n[2]), (strategy, i)


@pytest.mark.parametrize("fmt", (0, 1, 2))
@pytest.mark.parametrize("level", (0, 1, 6, 9))
def test_same_bytes_at_15_wrapped_calls(dev, fifteen, level, fmt):
    torch = dev.torch
    streams, src, offs, lens = fifteen
    wr = Wrapped(dev, src, offs, lens, fmt)
    for strategy in range(5):
        old, new = wr.streams2(dev, level, strategy, None), wr.streams2(dev, level, strategy, 15)
        assert old[0] == new[0] == 0, (strategy, old[0], new[0])
        assert torch.equal(old[1], new[1]) and torch.equal(old[2], new[2]), strategy
        assert int(old[1][:, 0].min()) > 0
        old, new = wr.members(dev, level, strategy, None), wr.members(dev, level, strategy, 15)
        assert old[0] == new[0] == 0, (strategy, old[0], new[0])
        assert all(torch.equal(a, b) for a, b in zip(old[1:], new[1:])), strategy
        assert 0 < int(old[1][-1]) <= wr.whole.numel()


# ---- a real small-window reader ------------------------------------------------------------------------------------------------
def _size_classes():
    out = {}
    for k, kind in enumerate(synth.CLASSES):
        part = synth.segment(kind, 256 << 10, np.random.default_rng([SIZE_SEED, k]))
        out[kind] = np.concatenate([part, np.zeros((256 << 10) - part.size, dtype=np.uint8)]).tobytes()
    return out


@pytest.fixture(scope="module")
def classes(dev):
    cl = _size_classes()
    host, offs, lens, _ = mc.pack([(b"", d) for d in cl.values()])
    return cl, dev.torch.from_numpy(host).cuda(), offs, lens


def _zlib_size(data, level, w):
    c = zlib.compressobj(level, zlib.DEFLATED, -w)
    return len(c.compress(data) + c.flush())


@pytest.mark.parametrize("level", (1, 6, 9))
@pytest.mark.parametrize("w", wc.WINDOWS)
def test_small_window_reader_and_size(dev, classes, w, level):
    cl, src, offs, lens = classes
    b = dev.dfl.StreamsBatch(src, offs, lens)
    b.run(level=level, window_bits=w)
    raws = [b.compressed(i) for i in range(b.n)]
    got = {}
    for (name, data), raw in zip(cl.items(), raws):
        assert wc.reader(-w, raw) == (data, True, b""), name
        got[name] = len(raw) / _zlib_size(data, level, w)
    for fmt, wbits in ((1, w), (2, 16 + w)):
        wr = Wrapped(dev, src, offs, lens, fmt)
        rc, res, dst = wr.streams2(dev, level, 0, w)
        assert rc == 0
        for i, (name, data) in enumerate(cl.items()):
            member = wr.member(res, dst, i)
            assert wc.reader(wbits, member) == (data, True, b""), (fmt, name)
            head = 2 if fmt == 1 else 10
            assert member[head:len(member) - (4 if fmt == 1 else 8)] == raws[i], (fmt, name)     # only the wrapper differs
            if fmt == 1:
                z = zlib.compressobj(level, zlib.DEFLATED, w)
                assert member[:2] == (z.compress(data[:64]) + z.flush())[:2], name
                if w >= 10:
                    with pytest.raises(zlib.error, match="invalid window size"):
                        wc.reader(w - 1, member)
    key = "%d-%d" % (w, level)
    print('    "%s": {%s},' % (key, ", ".join('"%s": %.4f' % kv for kv in got.items())))
    assert key in SIZE_RATIO, "no measured ratio for %s: %r" % (key, got)
    over = {n: (r, SIZE_RATIO[key][n]) for n, r in got.items() if r > SIZE_RATIO[key][n] + 0.01}
    assert not over, over


# ---- strategies ----------------------------------------------------------------------------------------------------------------
def test_strategies_at_window_10(dev):
    """Z_HUFFMAN_ONLY, Z_RLE and level 0 write distance 1 or none: the data bytes of 15, only the zlib header differs.
    Z_FIXED uses the window form: the cap holds and no block is dynamic."""
    cells = [c for c in wc.cells(10) if not c.history]
    streams = [c.data for c in cells] + [synth.silesia_like(300 << 10, seed=0xD37).tobytes()]
    host, offs, lens, _ = mc.pack([(b"", s) for s in streams])
    src = dev.torch.from_numpy(host).cuda()
    for level, strategy in ((6, 2), (6, 3), (1, 3)):
        assert dev.batch(streams, level, 10, strategy) == dev.batch(streams, level, 15, strategy), (level, strategy)
    wr = Wrapped(dev, src, offs, lens, 1)
    for level, strategy in ((6, 2), (6, 3), (0, 0), (0, 4)):
        rc10, res10, dst10 = wr.streams2(dev, level, strategy, 10)
        rc15, res15, dst15 = wr.streams2(dev, level, strategy, None)
        assert rc10 == rc15 == 0
        for i in range(wr.n):
            m10, m15 = wr.member(res10, dst10, i), wr.member(res15, dst15, i)
            assert m10[2:] == m15[2:] and m10[0] == 0x28 and m15[0] == 0x78, (level, strategy, i)
            assert (m10[0] * 256 + m10[1]) % 31 == 0 and m10[1] >> 6 == m15[1] >> 6
    for level in (1, 6, 9):
        fixed = dev.batch(streams, level, 10, 4)
        for k, (data, comp) in enumerate(zip(streams, fixed)):
            p = dp.parse(comp)
            assert p.data == data
            assert all(blk.btype != dp.DYNAMIC for blk in p.blocks), (level, k)
            assert mc.coverage(p, 0, 0).max_dist <= wc.cap(10), (level, k)
            assert wc.reader(-10, comp) == (data, True, b""), (level, k)
        for c, comp in zip(cells, fixed):
            assert wc.limits(c, dp.parse(comp)) is None, (level, c.name)


# ---- a function of the input ---------------------------------------------------------------------------------------------------
def test_output_is_a_function_of_the_input(dev):
    """w = 10, level 6: alone, alone again, among 24 others, and through deflate_dev -- the same bytes"""
    by_name = {c.name: c for c in wc.cells(10)}
    picks = [synth.silesia_like(300 << 10, seed=0xD37).tobytes(), by_name["w10/pos/m300-D762-at131072-tail300"].data,
             by_name["w10/pos/m16-D761-at61440-tail300"].data]
    others = [c.data for c in wc.cells(10) if not c.history and c.at < 62000][:24]
    assert len(others) == 24
    for k, data in enumerate(picks):
        first, again = dev.batch([data], 6, 10), dev.batch([data], 6, 10)
        mixed = dev.batch(others[:5 * k + 3] + [data] + others[5 * k + 3:], 6, 10)
        assert wc.reader(-10, first[0]) == (data, True, b"")
        assert again == first and mixed[5 * k + 3] == first[0], k
        src = dev.torch.from_numpy(np.frombuffer(data + bytes(16), dtype=np.uint8).copy()).cuda()
        dst, n = dev.dfl.deflate_dev(src, level=6, length=len(data), window_bits=10)
        assert dst[:n].cpu().numpy().tobytes() == first[0], k


# ---- the members file -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (1, 2))
def test_members_file_at_window_12(dev, classes, fmt):
    torch, inf = dev.torch, dev.inf
    cl, src, offs, lens = classes
    wr = Wrapped(dev, src, offs, lens, fmt)
    rc, res, dst = wr.streams2(dev, 6, 0, 12)
    assert rc == 0
    want = [wr.member(res, dst, i) for i in range(wr.n)]
    rc, offsets, checks, whole = wr.members(dev, 6, 0, 12)
    assert rc == 0
    offsets, total = offsets.cpu().tolist(), sum(len(m) for m in want)
    assert offsets == np.concatenate([[0], np.cumsum([len(m) for m in want])]).tolist() and offsets[-1] == total
    file = whole[:total].cpu().numpy().tobytes()
    assert file == b"".join(want) and bool((whole[total:] == CANARY).all())
    plain = b"".join(cl.values())
    for i, data in enumerate(cl.values()):
        want_check = zlib.adler32(data) if fmt == 1 else zlib.crc32(data)
        assert int(checks[i]) & 0xffffffff == want_check
        assert wc.reader(12 if fmt == 1 else 28, file[offsets[i]:offsets[i + 1]]) == (data, True, b"")
    back = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    file_dev = whole[:total].clone()
    if fmt == 1:
        jobs = inf.packed_jobs(file_dev, offsets[:-1], [len(m) for m in want])
        out_offs = torch.zeros(wr.n + 1, dtype=torch.int64, device="cuda")
        rows = torch.zeros((wr.n, 4), dtype=torch.int32, device="cuda")
        assert inf.uncompress_packed_dev(1, jobs, wr.n, back, out_offs, rows) == 0
        torch.cuda.synchronize()
        assert out_offs.cpu().tolist() == [i * (256 << 10) for i in range(wr.n + 1)]
        assert rows.cpu()[:, 2].tolist() == [1] * wr.n
    else:
        st, produced, used, members, nmembers, _ = inf.gunzip_members_dev(file_dev, back)
        assert (st, produced, used, nmembers) == (1, len(plain), total, wr.n), (st, produced, used, nmembers)
        assert [m[0] for m in members] == offsets[:-1]
    assert back[:len(plain)].cpu().numpy().tobytes() == plain


# ---- the refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(dev, classes):
    torch = dev.torch
    cl, src, offs, lens = classes
    refused = [(fmt, wb) for fmt in (0, 1, 2) for wb in (7, 16, 0, -15)] + [(0, 8), (2, 8)]
    for fmt, wb in refused:
        wr = Wrapped(dev, src, offs[:2], lens[:2], fmt)
        assert wr.streams2(dev, 6, 0, wb)[0] == EINVAL and wr.untouched(), (fmt, wb)
        assert wr.members(dev, 6, 0, wb)[0] == EINVAL and wr.untouched(), (fmt, wb)
    b = dev.dfl.StreamsBatch(src, offs[:2], lens[:2])
    for wb in (7, 16, 0, -15, 8):
        b.dst.fill_(CANARY)
        for i in range(b.n):
            b.out_lens[i] = 12345
        st = dev.rocm._stream_ptr(None)
        assert dev.lib.zng_rocm_deflate_window_streams_dev(6, 0, wb, C.byref(b.jobs), b.n, C.byref(b.out_lens), st) == EINVAL, wb
        out_len = C.c_size_t(12345)
        assert dev.lib.zng_rocm_deflate_window_block_dev(6, 0, wb, dev.rocm._dev_ptr(src, offs[0]), lens[0], 0, 0, dev.rocm._dev_ptr(b.dst),
                                                         int(b.dst.numel()), C.byref(out_len), st) == EINVAL, wb
        torch.cuda.synchronize()
        assert bool((b.dst == CANARY).all()) and [int(v) for v in b.out_lens] == [12345] * b.n and out_len.value == 12345, wb
    # 8 for the zlib format is 9, byte for byte
    wr = Wrapped(dev, src, offs, lens, 1)
    for level in (1, 6):
        eight, nine = wr.streams2(dev, level, 0, 8), wr.streams2(dev, level, 0, 9)
        assert eight[0] == nine[0] == 0 and torch.equal(eight[1], nine[1]) and torch.equal(eight[2], nine[2])
        assert wr.member(eight[1], eight[2], 0)[0] == 0x18
        eight, nine = wr.members(dev, level, 0, 8), wr.members(dev, level, 0, 9)
        assert eight[0] == nine[0] == 0 and all(torch.equal(a, b) for a, b in zip(eight[1:], nine[1:]))


# ---- the bound -----------------------------------------------------------------------------------------------------------------
def test_bound_holds_on_random_bytes_at_window_9(dev):
    data = np.random.default_rng(0xB0).integers(0, 256, size=256 << 10, dtype=np.uint8).tobytes()
    bound = dev.dfl.deflate_bound(len(data))
    for level in range(10):
        src = dev.torch.from_numpy(np.frombuffer(data + bytes(16), dtype=np.uint8).copy()).cuda()
        dst, n = dev.dfl.deflate_dev(src, level=level, length=len(data), window_bits=9)
        assert 0 < n <= bound, (level, n, bound)
        assert wc.reader(-9, dst[:n].cpu().numpy().tobytes()) == (data, True, b""), level
