"""The copy-resolution kernels of inflate_resolve.hip (K1 segments, K2 context groups and chain, K3 translate) on token streams
built token by token (tests/resolve_cases.py), through the C ABI: zng_rocm_inflate_resolve_dev, ..._resolve_window_dev and, for
the batch layout, zng_rocm_inflate_many.  Copies stand at chosen places against K1's flush mark, its ring, its literal window
and the previous segment; segment borders are placed by the test, under the host decoder's cutting policy and under one of
the test's own; the plaintext of the K2 / K3 streams has no period, so a lookup in the wrong table gives wrong bytes.  Every
comparison is exact, against resolve_cases.replay() (a byte replay of the token list; tests/test_resolve_cases_cpu.py holds it
to CPython's zlib), and every array passes resolve_cases.check_contract() before it is uploaded: the device stage has no error
channel, and nothing here gives it an invalid stream."""
import importlib
import zlib

import numpy as np
import pytest

import resolve_cases as rc
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu
CTX = rc.CTX
GUARD = 0xA5


@pytest.fixture(scope="module")
def inf():
    product().init()
    return importlib.import_module("zlib-ng_amd.inflate")


def _resolve(inf, s, window_call=None, sym_shift=0, out_shift=0):
    """one stream through the device stage; the window call when the stream has a window (or window_call says so)"""
    rc.check_contract(s)
    use_window = bool(s.window) if window_call is None else window_call
    assert use_window or not s.window
    dst = inf.resolve_arrays_dev(s.tokens, s.literals, s.segs, s.out_len, window=s.window if use_window else None,
                                 sym_shift=sym_shift, out_shift=out_shift, guard=64)
    host = dst.cpu().numpy()
    n = s.out_len
    assert host.size == out_shift + n + 64
    where = "%s (sym_shift %d, out_shift %d)" % (s.name, sym_shift, out_shift)
    assert (host[:out_shift] == GUARD).all(), "bytes in front of the output were written: " + where
    assert (host[out_shift + n:] == GUARD).all(), "bytes behind the output were written: " + where
    miss = s.first_mismatch(host[out_shift:out_shift + n].tobytes())
    assert miss is None, "%s, sym_shift %d, out_shift %d" % (miss, sym_shift, out_shift)


# ---- (a) K1: positions against the flush mark -------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["decoder", "placed"])
def test_k1_copies_and_runs_against_the_flush_mark(inf, policy):
    """far, overlapped and distance-1 copies whose source ends at, straddles or begins at the flush mark F = 2048, 4096, 6144
    (the read-back from HBM right behind the flush), and literal runs that begin with 2046 .. 2048 symbols unflushed"""
    _resolve(inf, rc.flush_mark_stream(policy))


# ---- (b) K1: the previous segment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["decoder", "placed"])
@pytest.mark.parametrize("window_len", [0, CTX])
def test_k1_copies_out_of_the_previous_segment(inf, policy, window_len):
    """copies at op 0, 1, dist - 1, dist, dist + 1 of segments s >= 1 (and of segment 0 behind a window): distance 32768 and 1
    at op 0, sources that cross the segment's first byte, overlapped copies entirely out of the previous segment"""
    _resolve(inf, rc.previous_segment_stream(policy, window_len))


# ---- (c) K1: literal window and token batches -------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["decoder", "placed"])
def test_k1_literal_window_and_token_batches(inf, policy):
    """first literal of a segment at every phase mod 16; runs that end on, begin on and cross multiples of 1024 literals;
    segments of 1, 63, 64, 65, 128, 129 tokens; one 32768-literal token; a segment of matches only"""
    _resolve(inf, rc.literal_window_stream(policy))


def test_k1_last_literals_of_the_array(inf):
    """a final segment that ends in a run of 1 .. 17 literals, the last bytes of `literals` (the bytewise tail of the staging)"""
    for s in rc.last_literals_streams():
        _resolve(inf, s)


# ---- (d) K2 and K3: segment counts and group borders ------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["decoder", "placed"])
@pytest.mark.parametrize("window_len", [0, CTX])
def test_k2_k3_alive_streams_at_the_group_borders(inf, policy, window_len):
    """matches only behind the first 32 KiB, distances of about 32768: every tail symbol stays a reference until the chain
    reaches the front.  nsegs 1 .. 193: no chain, the chain's early return, one and two steps of it, a last group of one tail"""
    for nsegs in rc.ALIVE_NSEGS:
        _resolve(inf, rc.alive_case(policy, window_len, nsegs))


def test_k2_k3_full_last_segment_and_empty_last_segment(inf):
    """the stream ends exactly where a segment does: as a last segment of full size, and with an empty segment behind it (what
    the decoder writes when a literal or a match fills the last segment)"""
    for policy in ("decoder", "placed"):
        for nsegs in (2, 65, 66):
            s = rc.alive_case(policy, 0, nsegs, last_tokens=None)
            _resolve(inf, s)
            segs = np.concatenate((s.segs, s.segs[-3:]))
            _resolve(inf, rc.Stream(s.name + "/empty_last", s.tokens, s.literals, segs, s.window, s.marks))


# ---- (e) K3: alignment ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("end", range(16))
def test_k3_every_alignment_of_symbols_and_destination(inf, end):
    """three segments, the last one short, out_len ending `end` bytes past a multiple of 16; d_symbols at every element
    offset 0 .. 7 crossed with d_out at every byte offset 0 .. 7, guard bytes around the destination"""
    s = rc.alignment_cases("placed")[end]
    assert s.nsegs == 3 and s.out_len % 16 == end
    for out_shift in range(8):
        for sym_shift in range(8):
            _resolve(inf, s, sym_shift=sym_shift, out_shift=out_shift)
    s = rc.alignment_cases("decoder")[end]
    for shift in range(8):
        _resolve(inf, s, sym_shift=shift, out_shift=7 - shift)


# ---- (f) windows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_len", rc.WINDOW_LENS)
def test_windows(inf, window_len):
    """zng_rocm_inflate_resolve_window_dev: a first token that reaches the window's first byte, overlapped copies out of the
    window, and 130 segments whose first is nothing but matches into the window (tail 0 resolved against the window)"""
    for s in rc.window_streams(window_len):
        _resolve(inf, s, window_call=True)
    _resolve(inf, rc.window_alive(window_len), window_call=True)


def test_streams_without_a_window_through_the_window_call(inf):
    for s in (rc.alive_case("placed", 0, 67), rc.literal_window_stream("decoder")):
        _resolve(inf, s, window_call=True)


def test_no_output_is_no_launch(inf):
    s = rc.Builder("decoder").finish("empty")
    _resolve(inf, s)
    _resolve(inf, s, window_call=True)


# ---- (g) the batch layout ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    streams = rc.batch_streams()
    for s in streams:
        rc.check_contract(s)
    comps = [rc.fixed_stream(s) for s in streams]
    for s, c in zip(streams, comps):                              # the second opinion
        d = zlib.decompressobj(-15, zdict=s.window) if s.window else zlib.decompressobj(-15)
        assert d.decompress(c) == s.expected() and d.eof, s.name
    return streams, comps


@pytest.mark.parametrize("nthreads", [1, 4])
def test_batch_layout_through_inflate_many(inf, batch, nthreads):
    """one zng_rocm_inflate_many call -- plaintexts of 0, 1, 3, 32767, 32768, 32769, 65541 bytes and alive streams of 3, 40 and
    30 segments, more than 65 segments in all: group borders inside a stream and next to stream borders, last segments that
    run on through the gap; windows of 1, 257 and 32768 bytes whose first byte is reached; destinations at all eight
    alignments inside one guard-filled tensor.  Which streams share a set of launches is decided by the dispatcher as the
    host threads deliver them, so a stream of 70 segments follows: its group border lies inside one stream whatever happens."""
    torch = torch_mod()
    streams, comps = batch
    assert sum(max(s.nsegs, 1) for s in streams) > 65
    assert {len(s.window) for s in streams} >= {0, 1, 257, CTX}
    starts, pos = [], 64
    for i, s in enumerate(streams):
        start = (pos + 7) // 8 * 8 + i % 8
        starts.append(start)
        pos = start + s.out_len + 24
    assert {(st % 8) for st, s in zip(starts, streams) if s.out_len} == set(range(8))
    big = torch.full((pos + 64,), GUARD, dtype=torch.uint8, device="cuda")
    dsts = [big[st:st + s.out_len] for st, s in zip(starts, streams)]
    windows = [torch.from_numpy(np.frombuffer(s.window, dtype=np.uint8).copy()).cuda() if s.window else None for s in streams]
    res = inf.inflate_many(comps, dsts, windows, nthreads=nthreads)
    host = big.cpu().numpy()
    covered = np.zeros(host.size, dtype=bool)
    for s, c, st, (status, out_len, in_used, msg) in zip(streams, comps, starts, res):
        assert (status, out_len, in_used) == (1, s.out_len, len(c)), (s.name, status, out_len, in_used, msg)
        miss = s.first_mismatch(host[st:st + s.out_len].tobytes())
        assert miss is None, "%s (nthreads %d, destination at %d mod 8)" % (miss, nthreads, st % 8)
        covered[st:st + s.out_len] = True
    assert (host[~covered] == GUARD).all(), "bytes outside the destinations were written at %s" % np.flatnonzero(
        ~covered & (host != GUARD))[:8]
