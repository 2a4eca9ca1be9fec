"""GPU: one preset dictionary shared by many small device-resident streams (zng_rocm_dict_create_dev,
zng_rocm_compress_streams_dict_dev, zng_rocm_uncompress_streams_dict_dev), raw and zlib framing, every step on the device.

  * foreign streams in: what CPython's zlib writes with zdict= (levels 1 / 6 / 9, raw and zlib) comes back bit-exact, bytes
    consumed = stream length, guard bytes intact -- for dictionaries of 1, 257, 32768 and 50000 bytes (the window is the tail,
    the DICTID covers everything);
  * the yardstick is the path the library had before: the same raw streams through zng_rocm_inflate_streams_dev with the
    window copied in front of every output give the same four result words, error rows included;
  * crafted streams put a copy exactly at, and one byte beyond, the dictionary's first byte;
  * the zlib judgement: another DICTID, FDICT clear, a damaged trailer, an output one byte short;
  * device streams out: three readers restore every message -- CPython with zdict=, the new call, the in-front path;
  * the dictionary is USED: on random bytes only dictionary matches can compress at all, and on a set of JSON-like records
    the device gains at least half of what CPython's level 1 gains from the same dictionary;
  * refusals, and a dictionary that outlives zng_rocm_shutdown()."""
import ctypes as C
import importlib
import json
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as craft
import synth
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu

DICT_LENS = (1, 257, 32768, 50000)
GUARD = 0xA5


@pytest.fixture(scope="module")
def mods():
    zr = product()
    zr.init()
    return zr, importlib.import_module("zlib-ng_amd.deflate"), importlib.import_module("zlib-ng_amd.inflate")


_WORDS = None


def _words():
    global _WORDS
    if _WORDS is None:
        rng = np.random.default_rng(2024)
        _WORDS = ["".join(chr(int(c)) for c in rng.integers(97, 123, size=int(k))) for k in rng.integers(3, 11, size=400)]
    return _WORDS


def _records(count, seed, lo=200, hi=2000):
    """JSON-like records of lo..hi bytes: the same keys and a shared vocabulary, different values"""
    rng = np.random.default_rng(seed)
    words = _words()
    out = []
    for k in range(count):
        want = int(rng.integers(lo, hi + 1))
        rec = {"id": int(rng.integers(0, 10 ** 9)), "user": words[int(rng.integers(0, 400))], "active": bool(rng.integers(0, 2)),
               "email": "%s@%s.example.com" % (words[int(rng.integers(0, 400))], words[int(rng.integers(0, 400))]),
               "created_at": "2024-%02d-%02dT%02d:%02d:%02dZ" % tuple(int(v) for v in rng.integers(1, 13, size=5)), "items": []}
        while len(json.dumps(rec)) < want:
            rec["items"].append({"sku": "%s-%04d" % (words[int(rng.integers(0, 400))], int(rng.integers(0, 10000))),
                                 "price": round(float(rng.integers(1, 100000)) / 100, 2), "currency": "EUR",
                                 "status": ("shipped", "pending", "returned")[int(rng.integers(0, 3))],
                                 "note": " ".join(words[int(v)] for v in rng.integers(0, 400, size=3))})
        out.append(json.dumps(rec).encode()[:want])                           # cut to size: JSON-like, not JSON
    return out


@pytest.fixture(scope="module")
def corpus():
    """the dictionaries, the messages and the record set: made once, never changed"""
    big = synth.silesia_like(100000, seed=77).tobytes()
    record_dict = b"".join(_records(60, seed=5))[-32768:]
    dicts = {}
    for n in DICT_LENS:
        text = b"".join(_records(80, seed=n))
        dicts[n] = (text * (n // len(text) + 1))[:n] if n != 32768 else record_dict
    return {"big": big, "dicts": dicts, "records": _records(200, seed=11), "record_dict": record_dict}


def _messages(D, big):
    tail = D[-min(len(D), 7):]
    return [b"", b"q", D[len(D) // 3:len(D) // 3 + min(len(D), 900)],      # every match source lies in the dictionary
            (tail * (600 // len(tail) + 1))[:600],                          # starts in the dictionary, runs into the stream: dist < len
            big]                                                            # longer than the LDS ring and than 32 KiB


def _pack(blobs, pad=3, first=1):
    offs, pos = [], first
    for b in blobs:
        offs.append(pos)
        pos += len(b) + pad
    host = np.full(pos + 64, 0x5c, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        host[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return host, offs


def _rows(inf, results):
    return [(r[2], r[0], r[1], inf.inflate_message(r[3])) for r in results]


def _uncompress_dict(inf, dic, blobs, caps, fmt):
    """the new call: streams at odd offsets, outputs at odd offsets with guard bytes around them"""
    torch = torch_mod()
    host, offs = _pack(blobs)
    out_off, pos = [], 7
    for c in caps:
        out_off.append(pos)
        pos += c + 9
    dst = torch.full((pos + 64,), GUARD, dtype=torch.uint8, device="cuda")
    b = inf.InflateDevBatch(torch.from_numpy(host).cuda(), offs, [len(x) for x in blobs], dst, out_off, caps)
    b.run_dict(fmt, dic)
    results = b.results.cpu().tolist()
    got = dst.cpu().numpy()
    assert got[:7].tolist() == [GUARD] * 7
    for o, c in zip(out_off, caps):
        assert got[o + c:o + c + 9].tolist() == [GUARD] * 9, "bytes behind out_cap were written"
    rows = _rows(inf, results)
    return results, rows, [got[o:o + r[1]].tobytes() for o, r in zip(out_off, rows)]


def _inflate_in_front(inf, window, blobs, caps):
    """the path the library had before: zng_rocm_inflate_streams_dev with the window copied in front of every output"""
    torch = torch_mod()
    W = len(window)
    host, offs = _pack(blobs)
    out_off, pos = [], 5
    for c in caps:
        out_off.append(pos + W)
        pos += W + c + 9
    image = np.full(pos + 64, GUARD, dtype=np.uint8)
    for o in out_off:
        image[o - W:o] = np.frombuffer(window, dtype=np.uint8)
    dst = torch.from_numpy(image).cuda()
    b = inf.InflateDevBatch(torch.from_numpy(host).cuda(), offs, [len(x) for x in blobs], dst, out_off, caps, dict_len=[W] * len(blobs))
    b.run()
    results = b.results.cpu().tolist()
    got = dst.cpu().numpy()
    rows = _rows(inf, results)
    return results, rows, [got[o:o + r[1]].tobytes() for o, r in zip(out_off, rows)]


def _raw_both(inf, dic, window, blobs, caps):
    """raw streams through the new call and through the yardstick: all four result words of every job agree"""
    results, rows, outs = _uncompress_dict(inf, dic, blobs, caps, 0)
    results_y, rows_y, outs_y = _inflate_in_front(inf, window, blobs, caps)
    assert results == results_y, [(i, a, b) for i, (a, b) in enumerate(zip(results, results_y)) if a != b]
    assert outs == outs_y
    return rows, outs


def _cpython(plain, level, wbits, D):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, zdict=D)
    return c.compress(plain) + c.flush()


def _fixed(tokens):
    bits = craft.Bits()
    craft.fixed_block(bits, tokens, True)
    bits.align()
    return bytes(bits.out)


# ---- foreign streams in ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dict_len", DICT_LENS)
def test_streams_of_cpython_with_zdict(mods, corpus, dict_len):
    zr, dfl, inf = mods
    D = corpus["dicts"][dict_len]
    window = D[-32768:]
    dic = dfl.Dictionary(D)
    try:
        assert dic.id == zlib.adler32(D) and dic.window == len(window)           # the DICTID covers ALL bytes, the window is the tail
        msgs = _messages(D, corpus["big"])
        want = [m for m in msgs for _ in (1, 6, 9)]
        raw = [_cpython(m, lvl, -15, D) for m in msgs for lvl in (1, 6, 9)]
        rows, outs = _raw_both(inf, dic, window, raw, [len(m) for m in want])
        for m, c, r, o in zip(want, raw, rows, outs):
            assert r == (1, len(m), len(c), "") and o == m
        zl = [_cpython(m, lvl, 15, D) for m in msgs for lvl in (1, 6, 9)]
        assert all(c[1] & 0x20 and c[2:6] == struct.pack(">I", dic.id) for c in zl)
        _, rows, outs = _uncompress_dict(inf, dic, zl, [len(m) for m in want], 1)
        for m, c, r, o in zip(want, zl, rows, outs):
            assert r == (1, len(m), len(c), "") and o == m
    finally:
        dic.close()


# ---- crafted inflate streams -----------------------------------------------------------------------------------------------
def test_copies_at_and_beyond_the_first_byte_of_the_dictionary(mods, corpus):
    zr, dfl, inf = mods
    for dict_len in (257, 32768, 50000):
        D = corpus["dicts"][dict_len]
        window = D[-32768:]
        W = len(window)
        dic = dfl.Dictionary(D)
        try:
            lits = [("L", b) for b in b"hello"]
            cases = [[("M", 3, W)], [("M", 258, W)], lits + [("M", 4, W)], lits + [("M", 10, 5)]]
            if W + 5 <= 32768:                                                # (a distance code reaches 32768)
                cases.append(lits + [("M", 4, 5 + W)])
            wants = [craft.replay(t, history=window) for t in cases]
            assert wants[0] == window[:3] and wants[2] == b"hello" + window[5:9]
            assert W + 5 > 32768 or wants[4] == b"hello" + window[:4]
            blobs, caps = [_fixed(t) for t in cases], [len(w) for w in wants]
            if W < 32768:                                                     # one byte too far (a distance code reaches 32768)
                blobs += [_fixed([("M", 3, W + 1)]), _fixed(lits + [("M", 4, 5 + W + 1)])]
                caps += [16, 16]
            rows, outs = _raw_both(inf, dic, window, blobs, caps)
            for w, c, r, o in zip(wants, blobs, rows, outs):
                assert r == (1, len(w), len(c), "") and o == w
            for r in rows[len(wants):]:
                assert (r[0], r[3]) == (-3, "invalid distance too far back"), r
        finally:
            dic.close()
    # a window of one byte: distance 1 at the first output byte reads it, distance 2 is refused
    dic = dfl.Dictionary(b"Z")
    try:
        rows, outs = _raw_both(inf, dic, b"Z", [_fixed([("M", 5, 1)]), _fixed([("M", 3, 2)])], [5, 16])
        assert rows[0] == (1, 5, len(_fixed([("M", 5, 1)])), "") and outs[0] == b"ZZZZZ"
        assert (rows[1][0], rows[1][3]) == (-3, "invalid distance too far back")
    finally:
        dic.close()


# ---- the zlib judgement ----------------------------------------------------------------------------------------------------
def test_zlib_judgement(mods, corpus):
    zr, dfl, inf = mods
    D, other = corpus["dicts"][32768], corpus["dicts"][257]
    dic = dfl.Dictionary(D)
    try:
        p = D[5000:6000] + b"and something new" + D[100:400]
        good = _cpython(p, 6, 15, D)
        foreign = _cpython(p, 6, 15, other)                                   # written with another dictionary
        plain = zlib.compress(p, 6)                                           # FDICT clear
        reach = b"\x78\x01" + _fixed([("M", 3, 1)]) + struct.pack(">I", 1)   # FDICT clear and a copy from in front of the output
        damaged = good[:-1] + bytes([good[-1] ^ 0x10])
        blobs = [good, foreign, plain, reach, damaged, good, good[:4], good[:-2], good + b"more bytes"]
        caps = [len(p)] * len(blobs)
        caps[5] = len(p) - 1                                                  # one byte short
        results, rows, outs = _uncompress_dict(inf, dic, blobs, caps, 1)
        assert rows[0] == (1, len(p), len(good), "") and outs[0] == p
        assert rows[1] == (-3, 0, 6, "") and results[1][3] == 0               # the only -3 row with an empty message
        assert rows[2] == (1, len(p), len(plain), "") and outs[2] == p        # decoded without history
        assert (rows[3][0], rows[3][3]) == (-3, "invalid distance too far back")
        assert (rows[4][0], rows[4][3]) == (-3, "incorrect data check")
        assert rows[5][0] == -5 and rows[5][1] <= len(p) - 1 and outs[5] == p[:rows[5][1]]
        assert rows[6] == (-5, 0, 0, "input ended before the final block")   # the header ends inside the DICTID
        assert (rows[7][0], rows[7][3]) == (-5, "input ended before the final block")
        assert rows[8] == (1, len(p), len(good), "")                          # trailing bytes are not consumed
        # the call without a dictionary names what it lacks
        torch = torch_mod()
        host, offs = _pack([good])
        dst = torch.zeros(len(p) + 64, dtype=torch.uint8, device="cuda")
        b = inf.InflateDevBatch(torch.from_numpy(host).cuda(), offs, [len(good)], dst, [8], [len(p)])
        b.run_wrapped(1)
        assert b.rows()[0][0] == -3 and b.rows()[0][3] == "need dictionary"
    finally:
        dic.close()


# ---- device streams out ----------------------------------------------------------------------------------------------------
def _compress(dfl, dic, msgs, fmt):
    """zng_rocm_compress_streams_dict_dev (dic) or zng_rocm_compress_streams_dev (None) over messages at odd offsets;
    returns (result rows, the streams); what lies behind a stream in its slot must not have been written"""
    torch = torch_mod()
    host, offs = _pack(msgs, pad=5, first=3)
    wb = dfl.WrappedBatch(torch.from_numpy(host).cuda(), offs, [len(m) for m in msgs], fmt, for_dict=dic is not None)
    if dic is None:
        wb.run()
    else:
        wb.run_dict(dic)
    res = [[v & 0xffffffff for v in row] for row in wb.results.cpu().tolist()]
    out = wb.dst.cpu().numpy()
    blobs = []
    for i, (total, _) in enumerate(res):
        o = wb.out_off[i]
        assert total <= wb.bounds[i]
        blobs.append(out[o:o + total].tobytes())
        assert not out[o + total:o + wb.bounds[i]].any(), "bytes behind the stream were written"
    return res, blobs


def _check_device_streams(mods, D, msgs):
    zr, dfl, inf = mods
    window = D[-32768:]
    dic = dfl.Dictionary(D)
    try:
        for fmt in (0, 1):
            res, blobs = _compress(dfl, dic, msgs, fmt)
            for m, c, r in zip(msgs, blobs, res):
                assert r[1] == zlib.adler32(m)                                   # of the plaintext alone
                d = zlib.decompressobj(15 if fmt else -15, zdict=D)
                assert d.decompress(c) == m and d.eof and d.unused_data == b""
                if fmt:
                    assert c[:16] == b"\x78\x3f" + struct.pack(">I", zlib.adler32(D)) + b"\x00\x00\x00\xff\xff" * 2
                    assert c[-4:] == struct.pack(">I", zlib.adler32(m))
            _, rows, outs = _uncompress_dict(inf, dic, blobs, [len(m) for m in msgs], fmt)
            for m, c, r, o in zip(msgs, blobs, rows, outs):
                assert r == (1, len(m), len(c), "") and o == m
            raw = [c[16:-4] for c in blobs] if fmt else blobs
            _, rows, outs = _inflate_in_front(inf, window, raw, [len(m) for m in msgs])
            for m, c, r, o in zip(msgs, raw, rows, outs):
                assert r == (1, len(m), len(c), "") and o == m
    finally:
        dic.close()


@pytest.mark.parametrize("dict_len", DICT_LENS)
def test_device_written_streams_three_readers(mods, corpus, dict_len):
    D = corpus["dicts"][dict_len]
    extra = [D[-300:] + b"tail", D[:1] * 700, corpus["big"][:255], corpus["big"][:256], corpus["big"][:257], corpus["big"][:1031]]
    _check_device_streams(mods, D, _messages(D, corpus["big"]) + extra)


def test_device_written_records(mods, corpus):
    _check_device_streams(mods, corpus["record_dict"], corpus["records"])


# ---- the dictionary is used ------------------------------------------------------------------------------------------------
def test_dictionary_matches_on_random_bytes(mods):
    zr, dfl, inf = mods
    D = np.random.default_rng(404).integers(0, 256, size=32768, dtype=np.uint8).tobytes()
    msgs = [D[-1500:-500], D[-9000:-8000]]
    without, _ = _compress(dfl, None, msgs, 0)
    assert all(r[0] >= len(m) for r, m in zip(without, msgs))                 # random bytes: nothing to find in the message
    dic = dfl.Dictionary(D)
    try:
        res, blobs = _compress(dfl, dic, msgs, 0)
    finally:
        dic.close()
    for m, c, r in zip(msgs, blobs, res):
        print("random bytes: %d -> %d with the dictionary" % (len(m), r[0]))
        assert zlib.decompressobj(-15, zdict=D).decompress(c) == m
        assert r[0] < len(m) / 4, (r[0], len(m))


def test_dictionary_gain_on_records(mods, corpus):
    zr, dfl, inf = mods
    D, msgs = corpus["record_dict"], corpus["records"]
    assert len(msgs) == 200 and all(200 <= len(m) <= 2000 for m in msgs)

    def level1(m, zdict):
        c = zlib.compressobj(1, zlib.DEFLATED, -15, zdict=zdict) if zdict else zlib.compressobj(1, zlib.DEFLATED, -15)
        return len(c.compress(m) + c.flush())
    g = 1.0 - sum(level1(m, D) for m in msgs) / sum(level1(m, None) for m in msgs)
    without, _ = _compress(dfl, None, msgs, 0)
    dic = dfl.Dictionary(D)
    try:
        res, _ = _compress(dfl, dic, msgs, 0)
    finally:
        dic.close()
    t0, t1 = sum(r[0] for r in without), sum(r[0] for r in res)
    print("records: %d bytes; device %d -> %d with the dictionary (gain %.3f); CPython level 1 gain g = %.3f"
          % (sum(len(m) for m in msgs), t0, t1, 1.0 - t1 / t0, g))
    assert g > 0.05                                                           # the set is one a dictionary helps
    assert t1 <= t0 * (1.0 - g / 2.0), (t0, t1, g)


# ---- refusals and the object's life ----------------------------------------------------------------------------------------
def _raw_calls(zr, dfl, inf, dic_handle, fmt, dict_len=0, flags=0):
    """both calls through ctypes with one small job each; returns their return values and whether the results were touched"""
    torch = torch_mod()
    lib = zr.lib()
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    res = torch.full((4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    cj = (dfl.StreamJob * 1)()
    cj[0].in_ptr, cj[0].out_ptr, cj[0].in_len, cj[0].out_cap = src.data_ptr() + 2048, dst.data_ptr(), 100, 4096
    cj[0].dict_len, cj[0].flags = dict_len, flags
    ij = (inf.InflateDevJob * 1)()
    ij[0].in_ptr, ij[0].out_ptr, ij[0].in_len, ij[0].out_cap = src.data_ptr(), dst.data_ptr() + 4096, 10, 100
    ij[0].dict_len, ij[0].flags = dict_len, flags
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc_c = lib.zng_rocm_compress_streams_dict_dev(fmt, dic_handle, C.byref(cj), 1, C.c_void_p(res.data_ptr()), st)
    rc_u = lib.zng_rocm_uncompress_streams_dict_dev(fmt, dic_handle, C.byref(ij), 1, C.c_void_p(res.data_ptr()), st)
    torch.cuda.synchronize()
    return rc_c, rc_u, res.cpu().tolist() == [0x5a5a5a5a] * 4 and not dst.cpu().numpy().any()


def test_refusals(mods, corpus):
    zr, dfl, inf = mods
    dic = dfl.Dictionary(corpus["dicts"][257])
    try:
        assert _raw_calls(zr, dfl, inf, dic.h, 2) == (-3, -3, True)             # gzip has no dictionary
        assert _raw_calls(zr, dfl, inf, dic.h, -1) == (-3, -3, True)
        assert _raw_calls(zr, dfl, inf, None, 0) == (-3, -3, True)              # no object
        assert _raw_calls(zr, dfl, inf, None, 1) == (-3, -3, True)
        assert _raw_calls(zr, dfl, inf, dic.h, 0, dict_len=16) == (-3, -3, True)     # the history is the object's
        assert _raw_calls(zr, dfl, inf, dic.h, 1, dict_len=16) == (-3, -3, True)
        assert _raw_calls(zr, dfl, inf, dic.h, 1, flags=1) == (-3, -3, True)    # block flags: raw streams only
        rc_c, rc_u, _ = _raw_calls(zr, dfl, inf, dic.h, 0, flags=3)             # ... where the compress side takes them
        assert (rc_c, rc_u) == (0, -3)
        torch = torch_mod()
        h = C.c_void_p(99)
        buf = torch.zeros(16, dtype=torch.uint8, device="cuda")
        assert zr.lib().zng_rocm_dict_create_dev(C.c_void_p(buf.data_ptr()), 0, C.byref(h), None) == -3 and not h.value
        h = C.c_void_p(99)
        assert zr.lib().zng_rocm_dict_create_dev(None, 16, C.byref(h), None) == -3 and not h.value
    finally:
        dic.close()


def test_dictionary_after_shutdown(mods, corpus):
    """runs last in this file: the context goes away under a live object and comes back"""
    zr, dfl, inf = mods
    D = corpus["dicts"][257]
    dic = dfl.Dictionary(D)
    assert _raw_calls(zr, dfl, inf, dic.h, 0)[:2] == (0, 0)
    torch_mod().cuda.synchronize()
    assert zr.lib().zng_rocm_shutdown() == 0
    try:
        assert _raw_calls(zr, dfl, inf, dic.h, 0) == (-1, -1, True)
        assert _raw_calls(zr, dfl, inf, dic.h, 1) == (-1, -1, True)
    finally:
        zr.init()
    assert _raw_calls(zr, dfl, inf, dic.h, 0) == (-1, -1, True)               # an object of the context that is gone
    dic.close()                                                               # ... is still freed without trouble
    fresh = dfl.Dictionary(D)
    try:
        assert fresh.id == zlib.adler32(D)
        res, blobs = _compress(dfl, fresh, [D[10:200]], 1)
        assert zlib.decompressobj(15, zdict=D).decompress(blobs[0]) == D[10:200]
    finally:
        fresh.close()
