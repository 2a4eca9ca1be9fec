"""zlib (RFC 1950) and gzip (RFC 1952) members through the LARGE device inflaters: zng_rocm_uncompress_large_streams_dev (a
batch, rounds of zng_rocm_inflate_large_streams_dev on the payloads) and zng_rocm_uncompress_large_dev (one member of any
length, zng_rocm_inflate_large_pieces_dev on the payload).  What is replaced is inflate()'s work in front of and behind the
deflate data: the header states (inflate.c:509-715) and the check value / length compare (inflate.c:1105-1147).
Oracles: for everything the wrapper does not touch, the raw call on the payload alone in a call of its own; for the wrapper,
CPython's zlib (the texts of the header and trailer errors, Z_NEED_DICT) and the plaintext."""
import ctypes as C
import importlib
import struct
import zlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

from wrapped_members import (MiB, SUB, ODDS, Member, place as _place, plain as _plain, raw as _raw, trailer as _trailer,  # noqa: F401
                             gzip_file as _gzip_file, handmade as _handmade, wrap as _wrap, mixed as _mixed)


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return (torch, importlib.import_module("zlib-ng_amd.inflate"), importlib.import_module("zlib-ng_amd.deflate"),
            importlib.import_module("zlib-ng_amd.oneshot"), zr)


def _guards_intact(m, whole):
    return int(whole[m.odd + m.cap:].min()) == 0xAB and int(whole[:m.odd].min()) == 0xAB


def _framed(torch, inf, fmt, members, subblock=False, round_bytes=0, stream=None):
    bufs = [m.dst(torch) for m in members]
    torch.cuda.synchronize()
    rc, rows, rounds, launches = inf.uncompress_large_streams_dev(fmt, [m.src for m in members], [b[1] for b in bufs],
                                                                  dicts=[m.zdict for m in members], round_bytes=round_bytes,
                                                                  subblock=subblock, stream=stream)
    return rc, rows, rounds, launches, bufs


def _raw_on_payloads(torch, inf, fmt, members, subblock=False, dicts=None):
    """the reference: the raw batch call on the bytes behind every header (trailer and whatever follows included, as the
    patched jobs have them), in a call of its own"""
    hl = []
    for m in members:
        st, n, _, _, msg = inf.wrapper_parse(fmt, m.data)
        assert st in (0, 2), (m.name, st, msg)
        hl.append(n)
    bufs = [m.dst(torch) for m in members]
    torch.cuda.synchronize()
    rc, rows, rounds, launches = inf.inflate_large_streams_dev([m.src[h:] for m, h in zip(members, hl)], [b[1] for b in bufs],
                                                               windows=dicts, subblock=subblock)
    assert rc == 0
    return rows, rounds, launches, hl


@pytest.fixture(scope="module")
def mixed(mods):
    torch, inf, dfl, one, _ = mods
    return {fmt: _mixed(torch, dfl, one, fmt) for fmt in (1, 2)}


@pytest.mark.parametrize("subblock", [False, True])
@pytest.mark.parametrize("fmt", [1, 2])
def test_mixed_batch(mods, mixed, fmt, subblock):
    torch, inf, _, _, _ = mods
    ms = mixed[fmt]
    raw_rows, raw_rounds, raw_launches, hl = _raw_on_payloads(torch, inf, fmt, ms, subblock)
    rc, rows, rounds, launches, bufs = _framed(torch, inf, fmt, ms, subblock)
    assert rc == 0
    tail = 4 if fmt == 1 else 8
    for m, row, raw, h, (whole, dst) in zip(ms, rows, raw_rows, hl, bufs):
        assert row[:4] == (1, len(m.plain), m.first, None), (m.name, row, raw)
        assert raw[0] == 1 and raw[2] + h + tail == m.first, (m.name, raw, h)
        assert dst[:row[1]].cpu().numpy().tobytes() == m.plain, m.name
        assert _guards_intact(m, whole), m.name
        assert (row[4] > 0) == (raw[4] > 0), (m.name, row, raw)
    assert (rounds, launches) == (raw_rounds, raw_launches)
    assert sum(1 for r in rows if r[4] > 0) >= 8, rows


def _bad_headers(fmt, good):
    """(name, member bytes, text) for every header refusal of the format"""
    out = []
    if fmt == 1:
        out.append(("header-check", bytes([good[0], good[1] ^ 1]) + good[2:], "incorrect header check"))
        for name, cmf, text in (("method", 0x77, "unknown compression method"), ("window", 0x88, "invalid window size")):
            flg = 31 - (cmf << 8) % 31
            out.append((name, bytes([cmf, flg]) + good[2:], text))
    else:
        out.append(("magic", b"\x1f\x8c" + good[2:], "incorrect header check"))
        out.append(("zlib-member-as-gzip", zlib.compress(b"abc" * 1000), "incorrect header check"))
        out.append(("method", good[:2] + b"\x07" + good[3:], "unknown compression method"))
        out.append(("unknown-flags", good[:3] + bytes([good[3] | 0x20]) + good[4:], "unknown header flags set"))
    return out


@pytest.mark.parametrize("fmt", [1, 2])
def test_trouble_between_regular_neighbours(mods, fmt):
    torch, inf, _, _, zr = mods
    tail = 4 if fmt == 1 else 8
    p = _plain(4, 300)
    good = zlib.compress(p, 6) if fmt == 1 else _handmade(p)
    st, hl, _, _, _ = inf.wrapper_parse(fmt, good)
    assert st == 0
    # the CPython oracle for the wrapper texts
    def cpython_text(data):
        try:
            zlib.decompressobj(15 if fmt == 1 else 31).decompress(data)
        except zlib.error as e:
            return str(e)
        return None

    trouble, expect = [], {}

    def add(name, data, row=None, cap=None):
        trouble.append(Member(torch, name, data, None, ODDS[len(trouble) % 8], cap=len(p) if cap is None else cap))
        expect[name] = row

    for name, data, text in _bad_headers(fmt, good):
        assert text in cpython_text(data), (name, cpython_text(data))
        add(name, data, (-3, 0, None, text))
    if fmt == 2:
        bad = bytearray(good)
        bad[hl - 1] ^= 0x40
        assert "header crc mismatch" in cpython_text(bytes(bad))
        add("wrong-fhcrc", bad, (-3, 0, None, "header crc mismatch"))
    bad = bytearray(good)
    bad[len(good) - tail] ^= 0x01
    assert "incorrect data check" in cpython_text(bytes(bad))
    add("flipped-check", bad, (-3, len(p), None, "incorrect data check"))
    if fmt == 2:
        bad = bytearray(good)
        bad[-1] ^= 0x80
        assert "incorrect length check" in cpython_text(bytes(bad))
        add("flipped-isize", bad, (-3, len(p), None, "incorrect length check"))
    cut = 1 if fmt == 1 else hl - 3
    add("cut-in-header", good[:cut], (-5, 0, cut, None))
    for t in ((1, 3) if fmt == 1 else (1, 7)):
        add("cut-after-%d-trailer-bytes" % t, good[:len(good) - tail + t], (-5, len(p), len(good) - tail + t, None))
    add("cut-in-payload", good[:len(good) // 2])
    # a flip inside the deflate data changes symbols, not the code: the decoders finish and the check value objects
    bad = bytearray(good)
    bad[hl + (len(good) - hl) // 2] ^= 0x10
    assert "incorrect data check" in cpython_text(bytes(bad))
    add("flip-in-deflate-data", bad, (-3, None, None, "incorrect data check"), cap=len(p) + 4096)   # a changed length may add bytes
    # ... and one in the first block's dynamic header is the decoder's own data error
    bad = bytearray(good)
    bad[hl + 2] ^= 0x5A
    assert "invalid" in cpython_text(bytes(bad)), cpython_text(bytes(bad))
    add("flip-in-block-header", bad)
    add("cap-one-short", good, cap=len(p) - 1)
    payload_trouble = [m for m in trouble if expect[m.name] is None]
    raw_rows, _, _, hls = _raw_on_payloads(torch, inf, fmt, payload_trouble)
    for m, raw, h in zip(payload_trouble, raw_rows, hls):
        assert raw[0] in (-3, -5), (m.name, raw)
        expect[m.name] = (raw[0], None, None, raw[3])                     # status and message of the raw call on the payload
    assert expect["flip-in-block-header"][0] == -3 and expect["cut-in-payload"][0] == -5 and expect["cap-one-short"][0] == -5
    plains = [_plain(4, 200 + k, extra=k) for k in range(3)]
    wrapped = [_wrap(fmt, q) for q in plains]
    regular = [Member(torch, "regular-%d" % k, wrapped[k % 3], plains[k % 3], ODDS[k % 8]) for k in range(len(trouble) + 1)]
    jobs = []
    for k, t in enumerate(trouble):
        jobs.append(regular[k])
        jobs.append(t)
    jobs.append(regular[len(trouble)])
    rc, rows, rounds, launches, bufs = _framed(torch, inf, fmt, jobs)
    assert rc == 0
    for m, row, (whole, dst) in zip(jobs, rows, bufs):
        assert _guards_intact(m, whole), m.name
        if m.plain is not None:
            assert row[:4] == (1, len(m.plain), len(m.data), None) and row[4] > 0, (m.name, row)
            assert dst.cpu().numpy().tobytes() == m.plain, m.name
            continue
        st, out_len, used, text = expect[m.name]
        assert (row[0], row[3]) == (st, text), (m.name, row, expect[m.name])
        if out_len is not None:
            assert row[1] == out_len, (m.name, row, expect[m.name])
        if used is not None:
            assert row[2] == used, (m.name, row, expect[m.name])
        assert row[2] <= len(m.data), (m.name, row)
        if m.name in ("flipped-check", "flipped-isize") or m.name.startswith("cut-after"):
            assert dst[:len(p)].cpu().numpy().tobytes() == p, m.name     # the plaintext is in place
        if out_len == 0:
            assert int(whole.min()) == 0xAB, m.name                       # a refused header writes nothing


def test_dictionary(mods):
    torch, inf, _, _, _ = mods
    d32 = _plain(1, 400)[:32768]
    d1k = _plain(1, 401)[:1000]

    def with_dict(plain, zdict, wbits=15):
        c = zlib.compressobj(6, zlib.DEFLATED, wbits, 8, zlib.Z_DEFAULT_STRATEGY, zdict)
        return c.compress(plain) + c.flush()

    p32 = d32[-5000:] + _plain(4, 402)
    p1k = d1k[-700:] + _plain(4, 403)
    m32, m1k = with_dict(p32, d32), with_dict(p1k, d1k)
    assert m32[1] & 0x20 and m1k[1] & 0x20
    nofdict = zlib.compress(b"")[:2] + with_dict(p32, d32, -15) + _trailer(1, p32)    # FDICT clear, payload needs the dictionary
    regular = _plain(4, 404)
    ms = [Member(torch, "dict-32768", m32, p32, 1, zdict=d32),
          Member(torch, "no-dictionary-given", m32, None, 3, cap=len(p32)),
          Member(torch, "regular", zlib.compress(regular, 6), regular, 5),
          Member(torch, "dictionary-one-byte-short", m32, None, 7, zdict=d32[:-1], cap=len(p32)),
          Member(torch, "dict-1000", m1k, p1k, 9, zdict=d1k),
          Member(torch, "fdict-clear-dictionary-given", nofdict, None, 11, zdict=d32, cap=len(p32)),
          Member(torch, "regular-with-a-dictionary-it-does-not-need", zlib.compress(regular, 6), regular, 13, zdict=d1k)]
    with pytest.raises(zlib.error, match="Error 2 "):
        zlib.decompressobj(15).decompress(m32)
    with pytest.raises(zlib.error, match="invalid distance too far back"):
        zlib.decompressobj(15, d32).decompress(nofdict)
    rc, rows, _, _, bufs = _framed(torch, inf, 1, ms)
    assert rc == 0
    by = {m.name: (row, whole, dst) for m, row, (whole, dst) in zip(ms, rows, bufs)}
    for m in ms:
        row, whole, dst = by[m.name]
        assert _guards_intact(m, whole), m.name
        if m.plain is not None:
            assert row[:4] == (1, len(m.plain), len(m.data), None), (m.name, row)
            assert dst.cpu().numpy().tobytes() == m.plain, m.name
    row, whole, _ = by["no-dictionary-given"]
    assert row[:4] == (2, 0, 6, None) and int(whole.min()) == 0xAB, row
    row, whole, _ = by["dictionary-one-byte-short"]
    assert (row[0], row[1], row[3]) == (-3, 0, None) and int(whole.min()) == 0xAB, row
    row, _, _ = by["fdict-clear-dictionary-given"]
    assert (row[0], row[3]) == (-3, "invalid distance too far back"), row
    # the single call: same answers
    m = ms[0]
    whole, dst = m.dst(torch)
    assert inf.uncompress_large_dev(1, m.src, dst, dict=m.zdict)[:3] == (1, len(p32), len(m32))
    assert dst.cpu().numpy().tobytes() == p32
    whole, dst = m.dst(torch)
    assert inf.uncompress_large_dev(1, m.src, dst)[:3] == (2, 0, 6) and int(whole.min()) == 0xAB


def test_long_header(mods):
    torch, inf, _, _, zr = mods
    p = _plain(4, 500)
    name = (np.random.default_rng(0x501).integers(1, 256, size=8 * MiB, dtype=np.uint8)).tobytes()
    head = bytes([0x1f, 0x8b, 8, 8 | 2, 0, 0, 0, 0, 0, 3]) + name + b"\0"
    head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    member = head + _raw(p) + _trailer(2, p)
    regular = _plain(4, 502)
    allname = bytes([0x1f, 0x8b, 8, 8 | 2, 0, 0, 0, 0, 0, 3]) + name * 8
    assert len(allname) > 64 * MiB
    wrongcrc = bytearray(member)
    wrongcrc[5 * MiB] = 7 if wrongcrc[5 * MiB] != 7 else 9                  # deep inside the name, under the FHCRC
    ms = [Member(torch, "8MiB-name", member, p, 3),
          Member(torch, "regular", _wrap(2, regular), regular, 5),
          Member(torch, "64MiB-all-name", allname, None, 7, cap=MiB),
          Member(torch, "8MiB-name-changed", wrongcrc, None, 9, cap=len(p))]
    rc, rows, _, _, bufs = _framed(torch, inf, 2, ms)
    assert rc == 0
    assert rows[0][:4] == (1, len(p), len(member), None), rows[0]
    assert bufs[0][1].cpu().numpy().tobytes() == p
    assert rows[1][:4] == (1, len(regular), len(ms[1].data), None) and rows[1][4] > 0, rows[1]
    assert rows[2][:4] == (-5, 0, len(allname), None), rows[2]
    assert (rows[3][0], rows[3][1], rows[3][3]) == (-3, 0, "header crc mismatch"), rows[3]
    for m, (whole, _) in zip(ms, bufs):
        assert _guards_intact(m, whole), m.name


def test_refusals_launch_nothing(mods, mixed):
    torch, inf, _, _, zr = mods
    stream = torch.cuda.Stream()
    before = inf.workspace_bytes(stream)

    def refused(fmt, mutate=None, **kw):
        some = mixed[fmt if fmt in (1, 2) else 1][:3]
        bufs = [m.dst(torch) for m in some]
        arr = inf.large_jobs([m.src for m in some], [b[1] for b in bufs], None)
        for a in arr:
            a.status, a.out_len, a.in_used, a.parts, a.subparts = 77, 78, 79, 80, 81
        if mutate:
            mutate(arr)
        rc, rows, _, _ = inf.uncompress_large_streams_dev(fmt, [m.src for m in some], None, jobs=arr, stream=stream, **kw)
        assert rc == -3, (fmt, kw, rc)                                    # ZNG_ROCM_EINVAL
        assert all(r[:3] == (77, 78, 79) and r[4:] == (80, 81) for r in rows), rows
        torch.cuda.synchronize()
        assert all(int(w.min()) == 0xAB for w, _ in bufs)
        assert inf.workspace_bytes(stream) == before

    def gzip_with_window(arr):
        arr[1].d_window, arr[1].window_len = arr[1].d_src, 100

    def window_too_long(arr):
        arr[1].d_window, arr[1].window_len = arr[1].d_src, 32769

    def null_src(arr):
        arr[2].d_src = None

    refused(-1)
    refused(3)
    refused(2, gzip_with_window)
    refused(1, window_too_long)
    refused(1, null_src)
    for fmt in (1, 2):
        refused(fmt, flags=2)
        refused(fmt, flags=0x80000001)
        refused(fmt, round_bytes=4 * MiB - 1)
        refused(fmt, round_bytes=2 << 30)
    # the single call
    m = mixed[2][0]
    whole, dst = m.dst(torch)
    for fmt, kw in ((-1, {}), (3, {}), (2, {"flags": 2}), (1, {"piece_bytes": 4 * MiB - 1}), (2, {"piece_bytes": (1 << 30) + 1}),
                    (2, {"dict": m.src[:100]})):
        got = inf.uncompress_large_dev(fmt, m.src, dst, stream=stream, **kw)
        assert got[:3] == (-3, 0, 0), (fmt, kw, got)
        torch.cuda.synchronize()
        assert int(whole.min()) == 0xAB and inf.workspace_bytes(stream) == before
    rc, rows, rounds, launches = inf.uncompress_large_streams_dev(2, [], [], stream=stream)
    assert (rc, rows, rounds, launches) == (0, [], 0, 0)


def test_format_0_is_the_raw_call(mods):
    torch, inf, _, _, _ = mods
    ms = []
    for k, (mib, level) in enumerate(((8, 6), (2, 1), (4, 9), (5, 6))):
        p = _plain(mib, 600 + k, extra=k)
        ms.append(Member(torch, "raw-%d" % k, _raw(p, level) + bytes(range(k)), p, ODDS[k]))
    damaged = bytearray(ms[0].data)
    damaged[len(damaged) // 2] ^= 0x10
    ms.append(Member(torch, "raw-damaged", damaged, None, 5, cap=8 * MiB))
    for subblock in (False, True):
        a = [m.dst(torch) for m in ms]
        b = [m.dst(torch) for m in ms]
        torch.cuda.synchronize()
        want = inf.inflate_large_streams_dev([m.src for m in ms], [x[1] for x in a], subblock=subblock)
        got = inf.uncompress_large_streams_dev(0, [m.src for m in ms], [x[1] for x in b], subblock=subblock)
        assert got == want
        for (wa, _), (wb, _), m in zip(a, b, ms):
            if m.plain is not None:
                assert torch.equal(wa, wb), m.name
    whole, dst = ms[0].dst(torch)
    whole2, dst2 = ms[0].dst(torch)
    assert inf.uncompress_large_dev(0, ms[0].src, dst) == inf.inflate_large_pieces_dev(ms[0].src, dst2)
    assert torch.equal(whole, whole2)


@pytest.mark.parametrize("fmt", [1, 2])
def test_single_call_against_uncompress2(mods, fmt):
    torch, inf, _, one, zr = mods
    p = _plain(64, 700 + fmt, extra=12345)
    member = zlib.compress(p, 6) if fmt == 1 else _handmade(p)
    m = Member(torch, "one-64MiB", member + b"behind", p, 7, first=len(member))
    ref = torch.zeros(len(p) + 16, dtype=torch.uint8, device="cuda")
    rc, dlen, slen, msg = one.uncompress2_dev(m.data, ref, fmt=fmt)
    assert (rc, dlen, slen) == (0, len(p), len(member)), (rc, dlen, slen, msg)
    for piece in (0, 4 * MiB):
        whole, dst = m.dst(torch)
        st, n, used, parts, pieces, host = inf.uncompress_large_dev(fmt, m.src, dst, piece_bytes=piece)
        assert (st, n, used) == (1, dlen, slen), (piece, st, n, used, zr.rocm.lib().zng_rocm_last_error())
        assert torch.equal(dst, ref[:len(p)]) and _guards_intact(m, whole)
        assert parts > 0 and (pieces > 1 if piece else pieces >= 1), (piece, parts, pieces)
    # the trailer of the single call
    bad = bytearray(member)
    bad[-1] ^= 0x01
    mb = Member(torch, "one-bad-trailer", bad, None, 9, cap=len(p))
    whole, dst = mb.dst(torch)
    st, n, used, _, _, _ = inf.uncompress_large_dev(fmt, mb.src, dst)
    text = zr.rocm.lib().zng_rocm_last_error().decode()
    assert (st, n) == (-3, len(p)) and text == ("incorrect data check" if fmt == 1 else "incorrect length check"), (st, n, text)


def test_isize_wraps(mods):
    """a gzip member of more than 4 GiB of plaintext: ISIZE is the length modulo 2^32"""
    torch, inf, _, _, zr = mods
    seg_plain = synth.silesia_like(32 << 20, seed=0x2A6B, seg_bytes=1 << 20)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    seg = c.compress(seg_plain.tobytes()) + c.flush(zlib.Z_SYNC_FLUSH)
    tiles = (1 << 32) // seg_plain.size + 1
    out_total = tiles * seg_plain.size
    assert (1 << 32) < out_total < (1 << 32) + (64 << 20)
    seg_crc = zlib.crc32(seg_plain.tobytes())
    crc = 0
    for _ in range(tiles):
        crc = zr.crc32_combine(crc, seg_crc, seg_plain.size)
    head = bytes([0x1f, 0x8b, 8, 8, 0, 0, 0, 0, 0, 3]) + b"big1\0"        # an odd header length
    total = len(head) + tiles * len(seg) + 2 + 8
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg_dev = torch.from_numpy(np.frombuffer(seg, dtype=np.uint8).copy()).cuda()
        plain_dev = torch.from_numpy(seg_plain).cuda()
        src = torch.empty(total, dtype=torch.uint8, device="cuda")
        src[:len(head)] = torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()).cuda()
        for i in range(tiles):
            src[len(head) + i * len(seg):len(head) + (i + 1) * len(seg)] = seg_dev
        at = len(head) + tiles * len(seg)
        src[at:at + 2] = torch.tensor([3, 0], dtype=torch.uint8, device="cuda")

        def trailer(crc_value, isize):
            src[at + 2:] = torch.from_numpy(np.frombuffer(struct.pack("<II", crc_value, isize), dtype=np.uint8).copy()).cuda()

        dst = torch.empty(out_total + 4096, dtype=torch.uint8, device="cuda")
        del seg_dev
    try:
        for crc_value, isize, want, text in ((crc, out_total & 0xffffffff, 1, None),
                                             (crc, (out_total & 0xffffffff) ^ 1, -3, "incorrect length check"),
                                             (crc ^ 1, out_total & 0xffffffff, -3, "incorrect data check")):
            with torch.cuda.stream(stream):
                trailer(crc_value, isize)
            stream.synchronize()
            st, n, used, parts, pieces, host = inf.uncompress_large_dev(2, src, dst, stream=stream)
            err = zr.rocm.lib().zng_rocm_last_error().decode()
            assert (st, n) == (want, out_total), (st, n, used, err)
            if want == 1:
                assert used == total and parts > 0, (used, total, parts)
                with torch.cuda.stream(stream):
                    bad = [i for i in range(tiles) if not torch.equal(dst[i * seg_plain.size:(i + 1) * seg_plain.size], plain_dev)]
                assert not bad, bad[:8]
            else:
                assert err == text, (err, text)
    finally:
        stream.synchronize()
        del src, dst
        zr.rocm.lib().zng_rocm_stream_release(C.c_void_p(stream.cuda_stream))
        torch.cuda.empty_cache()


def test_checksums_cut_dev(mods):
    """the check pass on its own (zng_rocm_checksums_cut_dev): few large messages, cut and folded, against CPython's
    adler32 / crc32 with the same seeds"""
    torch, _, _, _, zr = mods
    host = np.random.default_rng(0xC07).integers(0, 256, size=40 * MiB, dtype=np.uint8)
    host[3 * MiB:12 * MiB] = 0xff                                       # sums that wrap modulo 65521 often
    buf = torch.from_numpy(host).cuda()
    lens = [0, 1, SUB - 1, SUB, SUB + 1, 9 * MiB + 77, 17 * MiB + 3]
    offs, at = [], 5
    for n in lens:
        offs.append(at)
        at += n // 2 + 3                                                  # overlapping messages at odd addresses
    assert offs[-1] + lens[-1] <= host.size
    adlers = [1, 0x12345678 % 65521 | (777 << 16), 1, 0xfff0fff0, 1, 65520 | (65520 << 16), 1]
    crcs = [0, 0xdeadbeef, 0, 1, 0, 0xffffffff, 0]
    data = host.tobytes()
    for which in (1, 2, 3):
        out = torch.full((len(lens), 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        zr.checksums_cut_dev(which, buf, offs, lens, out, adlers=adlers, crcs=crcs)
        torch.cuda.synchronize()
        got = [[v & 0xffffffff for v in row] for row in out.tolist()]
        for k, (o, n) in enumerate(zip(offs, lens)):
            want = [zlib.adler32(data[o:o + n], adlers[k]) if which & 1 else 0x5A5A5A5A,
                    zlib.crc32(data[o:o + n], crcs[k]) if which & 2 else 0x5A5A5A5A]
            assert got[k] == want, (which, k, n, got[k], want)


@pytest.mark.parametrize("fmt", [1, 2])
def test_single_call_check_pass_in_chained_steps(mods, fmt):
    """the single call's check pass takes an output in steps (8 GiB each) with the seed chained through a device word; with
    the step lowered to 5 MiB + 3 by the library's test hook, a 24 MiB output takes five of them"""
    torch, inf, _, _, zr = mods
    hook = zr.rocm.lib().zng_rocm_debug_uncompress_large_chunk
    hook.restype, hook.argtypes = C.c_uint64, [C.c_uint64]
    p = _plain(24, 800 + fmt, extra=4321)
    member = _wrap(fmt, p)
    bad = bytearray(member)
    bad[-(4 if fmt == 1 else 8)] ^= 0x01
    m, mb = Member(torch, "steps", member, p, 5), Member(torch, "steps-bad-check", bad, None, 3, cap=len(p))
    assert hook(5 * MiB + 3) == 8 << 30
    try:
        whole, dst = m.dst(torch)
        assert inf.uncompress_large_dev(fmt, m.src, dst)[:3] == (1, len(p), len(member))
        assert dst.cpu().numpy().tobytes() == p and _guards_intact(m, whole)
        whole, dst = mb.dst(torch)
        assert inf.uncompress_large_dev(fmt, mb.src, dst)[:2] == (-3, len(p))
        assert zr.rocm.lib().zng_rocm_last_error().decode() == "incorrect data check"
    finally:
        assert hook(0) == 5 * MiB + 3
