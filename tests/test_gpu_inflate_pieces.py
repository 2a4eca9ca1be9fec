"""ONE device-resident raw stream decoded piece by piece (zng_rocm_inflate_large_pieces_dev): every result is compared with
zng_rocm_inflate_large_ex_dev on the same stream, or with the oracle inflater where the one-pass path cannot go (2 GiB of
input and more).  The loop decoded is inflate_fast (inffast_tpl.h:151-298) with the headers around it (inflate.c:735-917)."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

MIN_PIECE = 4 << 20


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), importlib.import_module("zlib-ng_amd.deflate"), zr


def _raw(plain, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(plain) + c.flush()


def _dev(torch, data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _err(zr):
    return zr.rocm.lib().zng_rocm_last_error().decode()


def _one_pass(torch, inf, zr, src, cap, sub, window=None):
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    st, n, used, _ = inf.inflate_large_dev(src, dst, window=window, subblock=sub)
    return st, n, used, dst, _err(zr)


def _pieces(torch, inf, zr, src, cap, piece, sub, window=None):
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    st, n, used, parts, passes, host = inf.inflate_large_pieces_dev(src, dst, piece_bytes=piece, window=window, subblock=sub)
    return st, n, used, dst, _err(zr), parts, passes, host


def _same(torch, inf, zr, comp, cap, piece, sub, window=None, tag=""):
    """pieces against the one-pass call: status, out_len, in_used, bytes, and the message of a data error"""
    src = _dev(torch, comp)
    st0, n0, used0, dst0, err0 = _one_pass(torch, inf, zr, src, cap, sub, window)
    st, n, used, dst, err, parts, passes, host = _pieces(torch, inf, zr, src, cap, piece, sub, window)
    assert (st, n, used) == (st0, n0, used0), (tag, piece, sub, (st, n, used), (st0, n0, used0), err, err0)
    assert torch.equal(dst, dst0), (tag, piece, sub)
    if st0 == -3:
        assert err == err0, (tag, err, err0)
    return parts, passes, host


_STREAMS = ["cpython1", "cpython6", "cpython9", "cpython_fixed", "own6", "quick"]


@pytest.fixture(scope="module")
def streams(mods):
    torch, _, dfl, _ = mods
    plain = synth.silesia_like(32 << 20, seed=0x91EC, seg_bytes=1 << 20)
    pb = plain.tobytes()
    out = {"cpython1": _raw(pb, 1), "cpython6": _raw(pb, 6), "cpython9": _raw(pb, 9),
           "cpython_fixed": _raw(pb, 6, zlib.Z_FIXED)}
    src_plain = torch.from_numpy(plain).cuda()
    comp, clen = dfl.deflate_dev(src_plain, level=6)
    out["own6"] = comp[:clen].cpu().numpy().tobytes()
    q = dfl.QuickBatch(src_plain, [0], [plain.size])
    q.run()
    torch.cuda.synchronize()
    out["quick"] = q.compressed(0)
    return pb, out


@pytest.mark.parametrize("name", _STREAMS)
@pytest.mark.parametrize("sub", [False, True])
def test_parity_with_one_pass(mods, streams, name, sub):
    torch, inf, _, zr = mods
    plain, comps = streams
    comp = comps[name]
    for piece in (MIN_PIECE, (5 << 20) + 12345, 0):
        parts, passes, host = _same(torch, inf, zr, comp, len(plain) + 4096, piece, sub, tag=name)
        # (a single fixed-code block, or fixed-code blocks without SUBBLOCK, offer the device nothing to cut at)
        if sub or name not in ("cpython_fixed", "quick"):
            assert host == 0, (name, piece, sub, host, _err(zr))
            if piece and piece < len(comp):
                assert passes >= -(-len(comp) // piece), (name, piece, passes)
        if sub and name == "cpython_fixed":
            assert inf.inflate_large_last_subparts() > 0


def test_irregular_streams_agree_with_one_pass(mods, streams):
    """bit flips and truncations at several offsets (in the second and in the last piece among them), a zlib trailer and
    garbage behind the stream, with 4 MiB pieces; status, message, out_len, in_used and bytes as the one-pass call has them"""
    torch, inf, _, zr = mods
    plain, comps = streams
    cap = len(plain) + 4096
    rng = np.random.default_rng(0x1BB)
    for name in ("cpython6", "cpython_fixed"):
        comp = comps[name]
        offs = [int(rng.integers(64, MIN_PIECE)), MIN_PIECE + 777777, len(comp) - 300000, len(comp) - 20]
        for sub in (False, True):
            for k, at in enumerate(offs):
                bad = bytearray(comp)
                bad[at] ^= 1 << (k % 8)
                _same(torch, inf, zr, bytes(bad), cap, MIN_PIECE, sub, tag=(name, "flip", at))
                _same(torch, inf, zr, comp[:at], cap, MIN_PIECE, sub, tag=(name, "cut", at))
            trailer = zlib.adler32(plain).to_bytes(4, "big") + bytes(rng.integers(0, 256, 1000, dtype=np.uint8))
            _same(torch, inf, zr, comp + trailer, cap, MIN_PIECE, sub, tag=(name, "trailer"))


def test_fixed_block_longer_than_the_piece(mods, streams):
    """the quick stream is ONE final fixed-code block, several pieces long"""
    torch, inf, _, zr = mods
    plain, comps = streams
    comp = comps["quick"]
    assert len(comp) > 2 * MIN_PIECE
    for sub in (False, True):
        _same(torch, inf, zr, comp, len(plain), MIN_PIECE, sub, tag="quick")
    st, n, used, dst, err, parts, passes, host = _pieces(torch, inf, zr, _dev(torch, comp), len(plain), MIN_PIECE, True)
    assert (st, n, used, host) == (1, len(plain), len(comp), 0), err
    assert passes >= 2 and inf.inflate_large_last_subparts() > 0


def test_small_dst_cap_writes_nothing_behind_it(mods, streams):
    torch, inf, _, zr = mods
    plain, comps = streams
    for name, sub in (("cpython6", False), ("cpython_fixed", True)):
        src = _dev(torch, comps[name])
        cap = len(plain) - 1
        dst = torch.full((len(plain) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        st, n, used, *_ = inf.inflate_large_pieces_dev(src, dst[:cap], piece_bytes=MIN_PIECE, subblock=sub)
        assert st == -5 and n > cap, (name, st, n)
        torch.cuda.synchronize()
        assert int(dst[cap:].min()) == 0xA5 and int(dst[cap:].max()) == 0xA5


def _splice_head():
    """a 32 KiB window, and 30000 incompressible bytes in five sync-flushed chunks behind it: several starts for the finder
    (stored blocks, sync markers), less than 32 KiB of output"""
    window = synth.silesia_like(32768, seed=0x3D1C).tobytes()
    p1 = np.random.default_rng(0x3D1D).integers(0, 256, 30000, dtype=np.uint8).tobytes()
    c1 = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, window)
    s1 = b"".join(c1.compress(p1[i:i + 6000]) + c1.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(p1), 6000))
    return window, p1, s1, (window + p1)[-32768:]


def _fixed_tail(hist, n, seed, final):
    """fixed-code blocks (which the finder cannot find) whose text begins with copies of both halves of the spliced
    history: the window's tail, then the first piece's output"""
    p2 = hist[:2768] + hist[5000:20000] + synth.silesia_like(n, seed=seed).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED, hist)
    return p2, c.compress(p2) + c.flush(zlib.Z_FINISH if final else zlib.Z_SYNC_FLUSH)


def _check_splice(torch, inf, zr, window, comp, plain, sub):
    import inflate_util
    st_o, _, ref, used_o = inflate_util.oracle_inflate_dict(comp, window, len(plain) + 16)
    assert (st_o, ref, used_o) == (1, plain, len(comp))
    st, n, used, dst, err, parts, passes, host = _pieces(torch, inf, zr, _dev(torch, comp), len(plain) + 16, MIN_PIECE, sub,
                                                         window=_dev(torch, window))
    assert (st, n, used) == (1, len(plain), len(comp)), (sub, st, n, used, err)
    assert dst[:n].cpu().numpy().tobytes() == plain, sub
    return passes, host, err


def test_history_splice_on_the_device(mods):
    """the first piece delivers the 30000 bytes in front of a fixed-code stretch that runs past its end (flags 0: no start
    inside it), and the second piece is the last one, so the device decodes it with the window's tail spliced with those
    30000 bytes as history; oracle: inflateSetDictionary"""
    torch, inf, _, zr = mods
    window, p1, s1, hist = _splice_head()
    p2, c2 = _fixed_tail(hist, 8 << 20, 0x3D1E, final=False)
    assert len(c2) < MIN_PIECE - (256 << 10)

    def tail(r):                                         # incompressible chunks, sync-flushed, then the final block
        raw = np.random.default_rng(0x3D1F).integers(0, 256, r, dtype=np.uint8).tobytes()
        c, q = zlib.compressobj(6, zlib.DEFLATED, -15), -(-r // 4)
        return raw, b"".join(c.compress(raw[i:i + q]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, r, q)) + c.flush()
    # the stretch and the tail together fill at most one piece, with the head in front more than one: the first pass ends
    # a quarter piece before the input's end, inside the stretch, and the second reaches the end
    r = MIN_PIECE - (8 << 10) - len(c2)
    p3, s3 = tail(r)
    p3, s3 = tail(r - (len(s3) - r))
    comp = s1 + c2 + s3
    assert len(comp) > MIN_PIECE and len(c2) + len(s3) <= MIN_PIECE and len(s3) < MIN_PIECE // 4
    passes, host, err = _check_splice(torch, inf, zr, window, comp, p1 + p2 + p3, False)
    assert (passes, host) == (2, 0), (passes, host, err)
    _check_splice(torch, inf, zr, window, comp, p1 + p2 + p3, True)


def test_history_splice_for_the_sequential_decoder(mods):
    """the same head in front of a fixed-code stretch several pieces long: the first pass delivers the head, the second
    cannot cut the stretch (flags 0), and the sequential decoder takes it from its first bit with the spliced history"""
    torch, inf, _, zr = mods
    window, p1, s1, hist = _splice_head()
    p2, c2 = _fixed_tail(hist, 16 << 20, 0x3D20, final=True)
    assert len(c2) > MIN_PIECE + (MIN_PIECE // 4)
    comp = s1 + c2
    passes, host, err = _check_splice(torch, inf, zr, window, comp, p1 + p2, False)
    assert (passes, host) == (1, len(c2)), (passes, host, len(c2), err)
    _check_splice(torch, inf, zr, window, comp, p1 + p2, True)


def test_refusals(mods, streams):
    torch, inf, _, zr = mods
    plain, comps = streams
    lib = zr.rocm.lib()
    src = _dev(torch, comps["cpython6"])
    dst = torch.full((len(plain),), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for piece, flags in ((0, 2), (0, 0x80000000), (MIN_PIECE, 3), (MIN_PIECE - 1, 0), (1, 1), (4096, 0), ((1 << 30) + 1, 0),
                         (1 << 40, 1), (2**64 - 1, 0)):
        out_len, in_used = C.c_uint64(77), C.c_size_t(77)
        rc = lib.zng_rocm_inflate_large_pieces_dev(zr.rocm._dev_ptr(src), int(src.numel()), None, 0, zr.rocm._dev_ptr(dst),
                                                   int(dst.numel()), C.byref(out_len), C.byref(in_used), piece, flags, None)
        assert rc == -3 and ("piece" in _err(zr) or "flag" in _err(zr)), (rc, _err(zr))    # ZNG_ROCM_EINVAL
        assert (out_len.value, in_used.value) == (0, 0), (piece, flags)
    torch.cuda.synchronize()
    assert int(dst.min()) == 0x5A and int(dst.max()) == 0x5A


def test_past_two_gib_of_input(mods):
    """sync-flushed copies of one segment, past 2^31 + 64 MiB of input, about 3 GiB of output: decoded on the device in
    64 MiB pieces on a fresh stream, with its scratch within the header's bound"""
    torch, inf, _, zr = mods
    seg_plain = synth.silesia_like(32 << 20, seed=0x2A6B, seg_bytes=1 << 20)
    rnd = np.random.default_rng(0x2A6C).integers(0, 256, size=seg_plain.size, dtype=np.uint8)
    mix = (np.arange(seg_plain.size) >> 20) % 2 == 1                       # every other MiB incompressible
    seg_plain = np.where(mix, rnd, seg_plain).astype(np.uint8)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    seg = c.compress(seg_plain.tobytes()) + c.flush(zlib.Z_SYNC_FLUSH)
    tiles = -(-((1 << 31) + (64 << 20)) // len(seg))
    total = tiles * len(seg) + 2
    out_total = tiles * seg_plain.size
    assert total > (1 << 31) + (64 << 20) and out_total < (7 << 29)
    stream = torch.cuda.Stream()
    piece = 64 << 20
    with torch.cuda.stream(stream):
        seg_dev = _dev(torch, seg)
        plain_dev = torch.from_numpy(seg_plain).cuda()
        src = torch.empty(total, dtype=torch.uint8, device="cuda")
        for i in range(tiles):
            src[i * len(seg):(i + 1) * len(seg)] = seg_dev
        src[tiles * len(seg):] = torch.tensor([3, 0], dtype=torch.uint8, device="cuda")
        dst = torch.empty(out_total + 4096, dtype=torch.uint8, device="cuda")
        del seg_dev
    stream.synchronize()
    try:
        st, n, used, parts, passes, host = inf.inflate_large_pieces_dev(src, dst, piece_bytes=piece, stream=stream)
        ws = inf.workspace_bytes(stream)
        assert (st, n, used, host) == (1, out_total, total, 0), (st, n, used, host, _err(zr))
        assert passes >= -(-total // piece)
        assert ws <= 256 * piece + (640 << 20) and ws < (24 << 30), ws
        with torch.cuda.stream(stream):
            bad = [i for i in range(tiles) if not torch.equal(dst[i * seg_plain.size:(i + 1) * seg_plain.size], plain_dev)]
        assert not bad, bad[:8]
    finally:
        stream.synchronize()
        del src, dst
        zr.rocm.lib().zng_rocm_stream_release(C.c_void_p(stream.cuda_stream))
        torch.cuda.empty_cache()
