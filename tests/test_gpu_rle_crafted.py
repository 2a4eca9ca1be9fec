"""GPU: the crafted runs of tests/rle_cases.py through rle_rows_kernel (deflate_rle.h), the front end of Z_RLE and
Z_HUFFMAN_ONLY, on every route that launches it -- one stream (zng_rocm_deflate_strategy_block_dev with dict_len), one ragged
batch (zng_rocm_deflate_strategy_streams_dev), the window forms, the hook and the wrapped members.  One fixture uploads all
cases once and keeps every one-stream and batch output; the window, hook and member routes run once each in their own test.
Every comparison is exact, and the
only expected values come from the greedy parse of deflate_rle.c (rle_cases.expected_tokens; CPython's zlib writes the same
tokens, tests/test_rle_cases_cpu.py), CPython's zlib as the reader, and tests/huffman_model.py:

  tokens    Z_RLE, one stream: the tokens are expected_tokens(case); CPython and the product's own inflater read the data back
  batch     every stream of one ragged batch has the one-stream bytes, in either order of the batch (the bitmap, distance and
            histogram scratch of a segment sits elsewhere then), for both strategies
  huffman   Z_HUFFMAN_ONLY: no match, one literal per byte, the same bytes at levels 1, 6 and 9
  blocks    every block covers the tokens that START in the plan's range [max(a, first + k BLOCK), min(b, first + (k + 1) BLOCK));
            its histograms are those tokens' (the kernel's snapshots held to its own bitmap), its codes cover them and cost
            the Huffman optimum
  window    windowBits 9, 12, 14 give the bytes of 15 for strategies 2 and 3 and for level 0
  hook      consecutive blocks of one stream out of the hook's 32 KiB ring, cut inside runs
  members   zlib and gzip members carry the one-stream bytes between header and trailer"""
import bisect
import ctypes as C
import importlib
import struct
import zlib

import numpy as np
import pytest

import deflate_parse as dp
import huffman_model as hm
import matcher_cases as mc
import rle_cases as rc
import strategy_util as su
from gpu_common import product, torch_mod
from rle_cases import BATCH, SEGMENT

pytestmark = pytest.mark.gpu

LIMITS = {"lit": 15, "dist": 15, "cl": 7}
STRATEGIES = (su.Z_RLE, su.Z_HUFFMAN_ONLY)
WINDOW_BITS = (9, 12, 14)
HOOK_HISTORY = 32768                                # kHist, hook.hip:28: what roll_history keeps, and the next block's dict_len


class Device:
    def __init__(self):
        zr = product()
        zr.init()
        self.torch = torch_mod()
        self.lib = zr.rocm.lib()
        self.dfl = importlib.import_module("zlib-ng_amd.deflate")
        self.inf = importlib.import_module("zlib-ng_amd.inflate")
        self.cases = rc.cases()
        self.index = {c.name: i for i, c in enumerate(self.cases)}
        self.host, self.offs, self.lens, self.dls = mc.pack([(c.history, c.data) for c in self.cases])
        assert self.host.size < 32 << 20                   # one call of this size cuts SEGMENT-byte segments
        self.src = self.torch.from_numpy(self.host).cuda()
        self.one = {s: [self.block(i, 6, s) for i in range(len(self.cases))] for s in STRATEGIES}
        self._batch, self._parsed = {}, {}

    def block(self, i, level, strategy, window_bits=15):
        """case i through the one-stream call"""
        dst, n = self.dfl.deflate_dev(self.src, level=level, length=self.lens[i], offset=self.offs[i], dict_len=self.dls[i],
                                      strategy=strategy, window_bits=window_bits)
        assert n <= self.dfl.deflate_bound(self.lens[i])
        return dst[:n].cpu().numpy().tobytes()

    def batch(self, strategy, level=6, reverse=False):
        """all cases as one ragged zng_rocm_deflate_strategy_streams_dev call -> the streams in the order of the cases"""
        key = (strategy, level, reverse)
        if key not in self._batch:
            order = list(range(len(self.cases)))[::-1] if reverse else list(range(len(self.cases)))
            if reverse:
                host, offs, lens, dls = mc.pack([(self.cases[i].history, self.cases[i].data) for i in order])
                src = self.torch.from_numpy(host).cuda()
            else:
                src, offs, lens, dls = self.src, self.offs, self.lens, self.dls
            b = self.dfl.StreamsBatch(src, offs, lens, dict_len=dls)
            rc_ = self.lib.zng_rocm_deflate_strategy_streams_dev(level, strategy, C.byref(b.jobs), b.n, C.byref(b.out_lens), None)
            assert rc_ == 0, key
            whole = b.dst.cpu().numpy()
            out = [None] * len(order)
            for k, i in enumerate(order):
                out[i] = whole[b.out_off[k]:b.out_off[k] + int(b.out_lens[k])].tobytes()
            self._batch[key] = out
        return self._batch[key]

    def parsed(self, strategy, i):
        if (strategy, i) not in self._parsed:
            c = self.cases[i]
            p = dp.parse(self.one[strategy][i], history=c.history)            # strict: an incomplete code set is an error
            assert p.data == c.data and (p.end_bit + 7) // 8 == len(self.one[strategy][i]), c.name
            self._parsed[strategy, i] = p
        return self._parsed[strategy, i]


@pytest.fixture(scope="module")
def dev():
    return Device()


def _inflate(comp, history=b""):
    d = zlib.decompressobj(-15, zdict=history) if history else zlib.decompressobj(-15)
    out = d.decompress(comp)
    assert d.eof and d.unused_data == b""
    return out


# ---- tokens -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_tokens(dev, family):
    """Z_RLE through zng_rocm_deflate_strategy_block_dev: token for token the greedy parse, per segment"""
    bad = []
    for c in rc.family(family):
        comp = dev.one[su.Z_RLE][dev.index[c.name]]
        got, want = su.tokens_of(comp, window_len=len(c.history)), rc.expected_tokens(c)
        if got != want:
            k = next((k for k, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
            at = c.dict_len + sum(t[1] if t[0] == 'm' else 1 for t in want[:k])
            bad.append((c.name, "token %d at position %d" % (k, at), got[k:k + 3], want[k:k + 3]))
    for b in bad:
        print("MISS", b)
    assert not bad, bad


def test_tokens_read_back(dev):
    """CPython inflates every Z_RLE stream to its data (with the history as zdict); the product's decode_tokens + resolve_dev
    gives the data of every stream without history (resolve_dev takes none)"""
    for i, c in enumerate(dev.cases):
        comp = dev.one[su.Z_RLE][i]
        assert _inflate(comp, c.history) == c.data, c.name
        if not c.history:
            dec = dev.inf.decode_tokens(comp)
            assert dec.status == 1, c.name
            assert dev.inf.resolve_dev(dec).cpu().numpy().tobytes() == c.data, c.name


# ---- batch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("reverse", [False, True])
def test_batch_has_the_one_stream_bytes(dev, strategy, reverse):
    got = dev.batch(strategy, 6, reverse)
    bad = [c.name for i, c in enumerate(dev.cases) if got[i] != dev.one[strategy][i]]
    assert not bad, bad


# ---- huffman-only -------------------------------------------------------------------------------------------------------------
def test_huffman_only(dev):
    """no block has a match, the literal tokens are the bytes, and the level makes no difference"""
    l1, l9 = dev.batch(su.Z_HUFFMAN_ONLY, 1), dev.batch(su.Z_HUFFMAN_ONLY, 9)
    for i, c in enumerate(dev.cases):
        comp = dev.one[su.Z_HUFFMAN_ONLY][i]
        assert _inflate(comp, c.history) == c.data, c.name
        dec = dev.inf.decode_tokens(comp, len(c.history))
        assert dec.status == 1 and not np.any(dec.tokens & 0x80000000), c.name
        assert int(dec.tokens.astype(np.int64).sum()) == len(c.data) == dec.literals.size, c.name
        assert dec.literals.tobytes() == c.data, c.name
        assert l1[i] == comp and l9[i] == comp, c.name


def test_rle_level_makes_no_difference(dev):
    l1, l9 = dev.batch(su.Z_RLE, 1), dev.batch(su.Z_RLE, 9)
    bad = [c.name for i, c in enumerate(dev.cases) if not l1[i] == l9[i] == dev.one[su.Z_RLE][i]]
    assert not bad, bad


# ---- blocks -------------------------------------------------------------------------------------------------------------------
def _model(case, strategy):
    """(start positions, end positions, literal/length symbols, is-match) of the tokens the strategy must write"""
    if strategy == su.Z_HUFFMAN_ONLY:
        pos = np.arange(case.dict_len, case.dict_len + len(case.data), dtype=np.int64)
        return pos, pos + 1, np.frombuffer(case.data, dtype=np.uint8).astype(np.int64), np.zeros(pos.size, dtype=bool)
    starts = rc.token_starts(case)
    pos = np.array([p for p, _ in starts], dtype=np.int64)
    length = np.array([t[1] if t[0] == 'm' else 1 for _, t in starts], dtype=np.int64)
    sym = np.array([257 + bisect.bisect_right(dp.LEN_BASE, t[1]) - 1 if t[0] == 'm' else t[1] for _, t in starts], dtype=np.int64)
    return pos, pos + length, sym, np.array([t[0] == 'm' for _, t in starts], dtype=bool)


def _sets(b):
    return {"lit": (b.lit_hist, b.lit_lens), "dist": (b.dist_hist, b.dist_lens), "cl": (b.cl_hist, b.cl_lens)}


@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_blocks(dev, strategy, family):
    kinds = set()
    for c in rc.family(family):
        p = dev.parsed(strategy, dev.index[c.name])
        blocks, ranges = dp.data_blocks(p), rc.block_ranges(c)
        assert len(blocks) == len(ranges), (c.name, len(blocks), ranges)
        pos, end, sym, is_match = _model(c, strategy)
        done = c.dict_len                                  # where the tokens of the blocks so far end
        for b, (lo, hi) in zip(blocks, ranges):
            k0, k1 = np.searchsorted(pos, lo), np.searchsorted(pos, hi)
            start = int(pos[k0]) if k1 > k0 else done
            done = int(end[k1 - 1]) if k1 > k0 else done
            where = (c.name, lo, hi)
            # the block's bytes: from its first token's start to its last token's end, which is behind hi when a match runs over
            assert (b.out_start + c.dict_len, b.out_end + c.dict_len) == (start, done), where
            assert hi <= done < hi + rc.CHAIN or k1 == k0, where
            if k1 > k0:
                assert int(pos[k1 - 1]) + 1 <= hi and start >= lo, where
            kinds.add(b.btype)
            if b.btype == dp.STORED:
                continue
            lit = np.bincount(sym[k0:k1], minlength=286)
            lit[256] += 1
            assert b.lit_hist == lit.tolist(), where
            assert b.dist_hist == [int(is_match[k0:k1].sum())] + [0] * 29, where
            if b.btype != dp.DYNAMIC:
                continue
            assert b.states == {"cl": "complete", "lit": "complete", "dist": "complete"}, where
            for which, (hist, lens) in _sets(b).items():
                assert max(lens) <= LIMITS[which], where
                used = [s for s, f in enumerate(hist) if f]
                coded = [s for s, n in enumerate(lens) if n]
                forced = [s for s in range(len(lens)) if s not in used][:max(0, 2 - len(used))]    # zlib's forced second code
                assert coded == sorted(used + forced), (where, which)
                if hm.min_max_depth(hist) <= LIMITS[which]:
                    assert hm.body_cost(hist, lens) == hm.optimal_cost(hist), (where, which)
    if family in ("segment", "block", "long"):
        assert dp.DYNAMIC in kinds, "no dynamic block in the family"


# ---- window -------------------------------------------------------------------------------------------------------------------
_STORED_AT_15 = {}                                  # level 0 at windowBits 15, shared by the three window tests


def _window_cases():
    out = rc.family("history") + rc.family("segment")
    return out + [rc.family(f)[0] for f in rc.FAMILIES if f not in ("history", "segment")]


@pytest.mark.parametrize("window_bits", WINDOW_BITS)
def test_window_forms_give_the_bytes_of_15(dev, window_bits):
    """zng_rocm_deflate_window_block_dev: Z_HUFFMAN_ONLY, Z_RLE and level 0 "give the bytes they give at 15" (zng_rocm.h)"""
    stored = _STORED_AT_15
    bad = []
    for c in _window_cases():
        i = dev.index[c.name]
        for s in STRATEGIES:
            if dev.block(i, 6, s, window_bits) != dev.one[s][i]:
                bad.append((c.name, s))
        if i not in stored:
            stored[i] = dev.block(i, 0, su.Z_RLE)
            assert _inflate(stored[i], c.history) == c.data, c.name
        if dev.block(i, 0, su.Z_RLE, window_bits) != stored[i]:
            bad.append((c.name, "level 0"))
    assert not bad, bad


# ---- hook ---------------------------------------------------------------------------------------------------------------------
HOOK_CASES = ("tail/batch+1-m1-r2", "segment/r3-t300", "long/L8449-s17")


def test_hook_blocks_cut_inside_runs(dev):
    """three cases' data as ONE stream through zng_rocm_hook_deflate_block_strategy, Z_RLE throughout, cut inside a run, one
    byte behind a run's start and on a BATCH multiple inside a run.  Block k sees dict_len = min(cut_k, 32768) bytes of history
    (zng_rocm_hook_deflate_block_window passes hist_len, which roll_history keeps at min(32768, hist_len + n)): its tokens are
    the greedy parse from cut_k on, cut into segments from a = that dict_len."""
    a, b, c = (rc.by_name(n) for n in HOOK_CASES)
    whole = a.data + b.data + c.data
    run_b = len(a.data) + b.edge["start"]
    run_c = len(a.data) + len(b.data) + c.edge["start"]
    on_batch = -(-(run_c + 300) // BATCH) * BATCH
    cuts = [0, a.edge["start"] + 101, run_b + 1, on_batch, len(whole)]
    brk = np.concatenate(([True], np.frombuffer(whole[1:], dtype=np.uint8) != np.frombuffer(whole[:-1], dtype=np.uint8)))
    assert not brk[cuts[1]] and brk[run_b] and not brk[run_b + 1] and not brk[on_batch] and on_batch < run_c + c.edge["length"]
    assert cuts == sorted(cuts) and cuts[2] - cuts[1] > SEGMENT and cuts[1] % 2       # more than a segment, from an odd dict_len

    h = C.c_void_p()
    assert dev.lib.zng_rocm_hook_create(C.byref(h), 1 << 20) == 0
    try:
        comp, cv, want = [], 1, []
        for k in range(len(cuts) - 1):
            piece = whole[cuts[k]:cuts[k + 1]]
            last = k == len(cuts) - 2
            buf = C.create_string_buffer(piece, len(piece))
            cap = dev.lib.zng_rocm_hook_deflate_bound(len(piece))
            out = C.create_string_buffer(cap)
            v, n = C.c_uint32(cv), C.c_size_t(0)
            flags = 0 if last else dev.dfl.BLOCK_NOT_FINAL | dev.dfl.BLOCK_SYNC_FLUSH
            st = dev.lib.zng_rocm_hook_deflate_block_strategy(h, 6, su.Z_RLE, C.addressof(buf), len(piece), flags, 1, C.byref(v),
                                                              C.addressof(out), cap, C.byref(n))
            assert st == 0, k
            comp.append(out.raw[:n.value])
            cv = int(v.value)
            assert cv == zlib.adler32(whole[:cuts[k + 1]]), k        # Adler-32 continues across the blocks
            hist = whole[cuts[k] - min(cuts[k], HOOK_HISTORY):cuts[k]]
            want.append(rc.stream_tokens(hist, piece))
    finally:
        dev.lib.zng_rocm_hook_destroy(h)
    # every block on its own: all but the last end with the sync marker and are not final
    for k, blk in enumerate(comp):
        hist = whole[cuts[k] - min(cuts[k], HOOK_HISTORY):cuts[k]]
        d = zlib.decompressobj(-15, zdict=hist) if hist else zlib.decompressobj(-15)
        assert d.decompress(blk) == whole[cuts[k]:cuts[k + 1]], k
        assert d.eof == (k == len(comp) - 1), k
        if k < len(comp) - 1:
            assert blk.endswith(b"\x00\x00\xff\xff"), k
        # a block that is not final ends on a byte behind its sync marker: the final empty static block makes it a whole stream
        got = su.tokens_of(blk if k == len(comp) - 1 else blk + b"\x03\x00", window_len=len(hist))
        assert got == want[k], k
    joined = b"".join(comp)
    assert _inflate(joined) == whole
    assert su.tokens_of(joined) == [t for w in want for t in w]


# ---- members ------------------------------------------------------------------------------------------------------------------
def _member_cases():
    return rc.family("plain") + rc.family("long") + rc.family("segment")


def _check_member(fmt, member, data, raw):
    head = (0, 2, 10)[fmt]
    tail = (0, 4, 8)[fmt]
    assert member[head:len(member) - tail] == raw                      # the one-stream bytes, so the one-stream tokens
    if fmt == 1:
        assert member[-4:] == struct.pack(">I", zlib.adler32(data))
    else:
        assert member[:4] == b"\x1f\x8b\x08\x00" and member[-8:] == struct.pack("<II", zlib.crc32(data), len(data))
    d = zlib.decompressobj((0, 15, 31)[fmt])
    assert d.decompress(member) == data and d.eof and d.unused_data == b""


@pytest.mark.parametrize("fmt", [1, 2])
def test_members(dev, fmt):
    """compress_streams2 and compress_members with Z_RLE: the body between header and trailer is the one-stream stream, the
    trailer is right and CPython reads every member"""
    torch, dfl = dev.torch, dev.dfl
    cases = _member_cases()
    idx = [dev.index[c.name] for c in cases]
    views = [dev.src[dev.offs[i]:dev.offs[i] + dev.lens[i]] for i in idx]
    caps = [(dfl.compress_streams2_bound(dev.lens[i], fmt) + 15) & ~15 for i in idx]
    starts = np.concatenate(([0], np.cumsum(caps))).tolist()
    arena = torch.zeros(starts[-1] + 16, dtype=torch.uint8, device="cuda")
    results = torch.zeros((len(idx), 2), dtype=torch.int32, device="cuda")
    jobs = dfl.stream_jobs(views, [arena[o:o + n] for o, n in zip(starts, caps)])
    assert dfl.compress_streams2_dev(jobs, len(idx), results, fmt, 6, su.Z_RLE) == 0
    torch.cuda.synchronize()
    host, res = arena.cpu().numpy(), results.cpu().tolist()
    for k, (c, i) in enumerate(zip(cases, idx)):
        n, check = int(res[k][0]), int(res[k][1]) & 0xffffffff
        assert check == (zlib.adler32(c.data) if fmt == 1 else zlib.crc32(c.data)), c.name
        _check_member(fmt, host[starts[k]:starts[k] + n].tobytes(), c.data, dev.one[su.Z_RLE][i])

    file_dev = torch.zeros(starts[-1] + 16, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(len(idx) + 1, dtype=torch.int64, device="cuda")
    checks = torch.zeros(len(idx), dtype=torch.int32, device="cuda")
    jobs = dfl.stream_jobs(views)
    assert dfl.compress_members_dev(jobs, len(idx), file_dev, offsets, fmt, 6, su.Z_RLE, 0, checks) == 0
    torch.cuda.synchronize()
    host, off, chk = file_dev.cpu().numpy(), offsets.cpu().tolist(), checks.cpu().tolist()
    assert off[0] == 0 and off[-1] <= file_dev.numel()
    for k, (c, i) in enumerate(zip(cases, idx)):
        assert int(chk[k]) & 0xffffffff == (zlib.adler32(c.data) if fmt == 1 else zlib.crc32(c.data)), c.name
        _check_member(fmt, host[off[k]:off[k + 1]].tobytes(), c.data, dev.one[su.Z_RLE][i])
