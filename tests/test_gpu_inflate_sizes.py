"""GPU: zng_rocm_inflate_sizes_dev (the sizing pass: a parse that stores nothing) and zng_rocm_uncompress_packed_dev (sizes,
places, decode and verification in one enqueue sequence) -- the read side of zng_rocm_compress_members_dev.

Expected values come from CPython's zlib, from the oracle inflater (inflate_util) and from the existing decode calls
(zng_rocm_inflate_streams_dev, zng_rocm_uncompress_streams_dev / _dict_dev), never from the new code.

One field departs from "the row the decode would write": the plaintext count of a stream that runs out of input (-5, "input
ended before the final block").  The decoder parses whole 32-bit words, so its partial count includes what the zero bits behind
the input decoded to and depends on where its flush tests fall (tests/test_gpu_inflate_dynamic.py leaves it out of its
comparison with the oracle).  The sizing pass documents another figure there -- the bytes of the symbols whose bits were all
input, which is what inflate() itself delivers for that input -- and that is what is checked: for every such row the count
EQUALS the length of the oracle's partial output and is no more than the decoder's, and where the decoder's count is exact
(a stored block cut inside its data, a cut on a block boundary) the whole row equals the decoder's.  Status, message and
consumed bytes of those rows are the decoder's like every other row's.

For a stream with a data error (-3) status and message are held against the oracle and the whole row against the decoder, as
the decoder's own tests do: the oracle consumes input a byte at a time and reports avail_in, so its consumed bytes at a fault
are not the bit position of the fault, and its partial output at a fault is whatever inflate_fast had written."""
import gzip
import importlib
import io
import json
import os
import struct
import threading
import zlib

import numpy as np
import pytest

import dynamic_cases as dc
import inflate_util
import ref_fixtures
import synth
import wrapper_cases
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "inflate_kat.json")))
GUARD = 0xA5
STARVED = "input ended before the final block"
FULL = "output buffer too small"


@pytest.fixture(scope="module")
def mods():
    zr = product()
    zr.init()
    return zr, importlib.import_module("zlib-ng_amd.deflate"), importlib.import_module("zlib-ng_amd.inflate")


def _raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, zdict=None):
    if zdict is None:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy, zdict)
    return c.compress(data) + c.flush()


def _lay(blobs):
    """one device image of the blobs: blob i at an offset that is i mod 4 (all four values of address & 3 occur; odd offsets
    among them), garbage -- not zeros -- behind every second one"""
    torch = torch_mod()
    offs, pos = [], 1
    for i, b in enumerate(blobs):
        while pos % 4 != i % 4:
            pos += 1
        offs.append(pos)
        pos += len(b) + 3
    host = np.zeros(pos + 64, dtype=np.uint8)
    for i, (o, b) in enumerate(zip(offs, blobs)):
        host[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        if i % 2:
            host[o + len(b):o + len(b) + 3] = (0x5c, 0xff, 0x93)
    if len(blobs) >= 4:
        assert {o & 3 for o in offs} == {0, 1, 2, 3}
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 4 == 0
    return dev, offs


def _sizes(inf, blobs, fmt, dict_len=None, dictionary=None, laid=None):
    """the sizing rows of the blobs; out / out_cap of the jobs are null and 0: the call must not look at them"""
    torch = torch_mod()
    src, offs = laid if laid is not None else _lay(blobs)
    b = inf.InflateDevBatch(src, offs, [len(x) for x in blobs], torch.empty(0, dtype=torch.uint8, device="cuda"),
                            [0] * len(blobs), [0] * len(blobs))
    for i in range(len(blobs)):
        b.jobs[i].out_ptr = None
        b.jobs[i].dict_len = 0 if dict_len is None else int(dict_len[i])
    b.results.fill_(0x5a5a5a5a)
    b.run_sizes(fmt, dictionary)
    return b.rows()


def _decode(inf, blobs, caps, fmt=0, dict_len=None, dictionary=None, laid=None):
    """the existing decode calls over the same image, every job with caps[i] bytes of room of its own (the room is never read
    back here: rows only); a job with dict_len gets that many bytes, of any value, in front of its output"""
    torch = torch_mod()
    src, offs = laid if laid is not None else _lay(blobs)
    dl = [0] * len(blobs) if dict_len is None else [int(d) for d in dict_len]
    out_off, pos = [], 0
    for c, d in zip(caps, dl):
        pos += d
        out_off.append(pos)
        pos += c
    dst = torch.empty(pos + 64, dtype=torch.uint8, device="cuda")
    b = inf.InflateDevBatch(src, offs, [len(x) for x in blobs], dst, out_off, caps, dl)
    if dictionary is not None:
        b.run_dict(fmt, dictionary)
    elif fmt:
        b.run_wrapped(fmt)
    else:
        b.run()
    return b.rows()


def _same(sized, decoded):
    """a sizing row against the decode's own row (see the module text for the count of a stream that ran out of input: never
    more than the decoder's)"""
    if sized[0] == -5 and sized[3] == STARVED:
        return (sized[0], sized[2], sized[3]) == (decoded[0], decoded[2], decoded[3]) and sized[1] <= decoded[1]
    return sized == decoded


def _starved_count_is_the_oracles(sized, oracle):
    """a row that ran out of input carries the bytes inflate() delivers for that input"""
    return not (sized[0] == -5 and sized[3] == STARVED) or sized[1] == len(oracle[2])


# ---- 1. raw streams: the oracle's verdict and the decoder's row -----------------------------------------------------------------
def _corpus():
    rng = np.random.default_rng(3)
    cases = {
        "mix": synth.silesia_like(1 << 20, seed=7, seg_bytes=256 << 10).tobytes(),
        "zeros": b"\0" * 300000,
        "period7": b"abcdefg" * 20000,
        "period300": bytes(rng.integers(0, 256, size=300, dtype=np.uint8)) * 900,
        "random": rng.integers(0, 256, size=200000, dtype=np.uint8).tobytes(),
        "empty": b"",
        "one": b"x",
        "far": rng.integers(0, 256, size=32768, dtype=np.uint8).tobytes() * 5,     # distance 32768 everywhere
        "text": (b"the quick brown fox jumps over the lazy dog; " * 3000)[:100001],
    }
    out = []
    for name, data in cases.items():
        for level, strat in ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
                             (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
            out.append(((name, level, strat), _raw(data, level, strat), data))
    return out


def test_corpus_sizes_are_the_plaintext_lengths(mods):
    """the corpus of tests/test_gpu_inflate_dev.py::test_corpus_levels_and_strategies: empty, one byte, several stored blocks,
    fixed, dynamic, RLE, huffman-only, distance 32768; streams of more than 512 and of more than 64 KiB compressed bytes"""
    zr, dfl, inf = mods
    corpus = _corpus()
    blobs = [s for _, s, _ in corpus]
    assert max(len(s) for s in blobs) > (64 << 10) and any(512 < len(s) < 4096 for s in blobs)
    assert any(len(p) > 65535 and s[0] & 6 == 0 for _, s, p in corpus)           # level 0: more than one stored block
    laid = _lay(blobs)
    rows = _sizes(inf, blobs, 0, laid=laid)
    for (nm, s, p), r in zip(corpus, rows):
        assert r == (1, len(p), len(s), ""), (nm, r)
    dec = _decode(inf, blobs, [len(p) for _, _, p in corpus], laid=laid)
    assert rows == dec


def test_crafted_streams_agree_with_the_oracle_and_the_decoder(mods):
    """every dynamic_cases valid and invalid case, the truncation sweep, the infcover rows and the reference's fixtures: status
    and message are the oracle's at a room of 70000; length and consumed bytes are the oracle's where the stream is complete;
    the whole row is the decoder's with that room; where the input ran out the count is the length of the oracle's partial
    output (see the module text)"""
    zr, dfl, inf = mods
    cap = 70000
    items = []                                                                   # (name, stream, history length, oracle verdict)
    for c in dc.valid_cases():
        h = c.history
        items.append((c.name, c.stream, len(h), inflate_util.oracle_inflate_dict(c.stream, h, cap) if h else inflate_util.oracle_inflate(c.stream, cap)))
    for x in dc.invalid_cases():
        items.append((x.name, x.stream, 0, inflate_util.oracle_inflate(x.stream, cap)))
    for s, e in dc.truncation_sweep():
        assert e[1] != FULL and len(e[2]) < dc.CAP                               # so the sweep's verdict at its own room is the verdict at 70000
        items.append(("sweep", s, 0, e))
    for r in KAT["rows"]:
        s = bytes(int(t, 16) for t in r["hex"].split())
        items.append(("infcover", s, 0, inflate_util.oracle_inflate(s, cap)))
    blobs = [it[1] for it in items]
    hist = [it[2] for it in items]
    laid = _lay(blobs)
    rows = _sizes(inf, blobs, 0, dict_len=hist, laid=laid)
    dec = _decode(inf, blobs, [cap] * len(blobs), dict_len=hist, laid=laid)
    differ = []
    for (name, s, h, (ost, omsg, oout, oused)), r, d in zip(items, rows, dec):
        ok = (r[0], r[3]) == (ost, omsg) and _same(r, d) and _starved_count_is_the_oracles(r, (ost, omsg, oout, oused))
        if ost == 1:
            ok = ok and (r[1], r[2]) == (len(oout), oused)
        if not ok:
            differ.append((name, s.hex()[:80], h, r, d, (ost, omsg, len(oout), oused)))
    assert not differ, (len(differ), differ[:5])
    assert sum(1 for it in items if it[3][0] == -3) > 50 and sum(1 for it in items if it[3][0] == 1) > 100
    starved = [r for r in rows if r[0] == -5 and r[3] == STARVED]
    assert len(starved) > 10000 and sum(1 for r in starved if r[1] > 0) > 1000   # the count of such rows is no constant


def test_truncated_counts_where_the_decoders_is_exact(mods):
    """a stored block cut inside its data, and a cut on a byte-aligned block boundary: nothing behind the input is decoded by
    anyone, so the sizing row, the decoder's row and the oracle's partial output agree in every field (zeros lie behind these
    streams: they stand at even places of the image, a complete empty block at the odd ones)"""
    zr, dfl, inf = mods
    rng = np.random.default_rng(17)
    noise = rng.integers(0, 256, size=100000, dtype=np.uint8).tobytes()
    stored = _raw(noise, 0)                                                      # stored blocks behind 5-byte headers
    text = synth.silesia_like(60000, seed=3).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    first = c.compress(text[:40000]) + c.flush(zlib.Z_FULL_FLUSH)                # ends on a byte, behind an empty stored block
    whole = first + c.compress(text[40000:]) + c.flush()
    assert zlib.decompress(whole, -15) == text
    n0 = stored[1] | stored[2] << 8                                              # LEN of the first stored block
    assert stored[0] == 0 and n0 == (stored[3] | stored[4] << 8) ^ 0xffff and 1000 < n0 < len(noise) - 1000
    cases = [(stored[:5 + 1], 1), (stored[:5 + 1000], 1000), (stored[:5 + n0], n0), (stored[:5 + n0 + 3], n0),
             (stored[:5 + n0 + 5 + 77], n0 + 77), (stored[:len(stored) - 1], len(noise) - 1), (first, 40000),
             (first[:-4], 40000)]                                                 # (the second: inside the empty stored block's LEN)
    filler = b"\x03\x00"                                                         # BFINAL, fixed codes, end of block
    blobs = [b for s, _ in cases for b in (s, filler)]
    laid = _lay(blobs)
    rows = _sizes(inf, blobs, 0, laid=laid)
    dec = _decode(inf, blobs, [100000] * len(blobs), laid=laid)
    for k, (s, n) in enumerate(cases):
        o = inflate_util.oracle_inflate(s, 100000)
        assert (o[0], len(o[2])) == (-5, n), (k, o[0], len(o[2]))
        r = rows[2 * k]
        assert (r[0], r[1], r[3]) == (-5, n, STARVED) and r == dec[2 * k], (k, r, dec[2 * k])
        assert rows[2 * k + 1] == (1, 0, 2, "") == dec[2 * k + 1]


def test_reference_fixtures_raw_payloads(mods):
    """the reference's own compressed fixtures, their raw deflate payloads cut out of the wrapper"""
    zr, dfl, inf = mods
    blobs, want = [], []
    for entry, data in ref_fixtures.compressed():
        if entry["format"] == "gzip":
            pos, _ = ref_fixtures.gzip_payload(data)
            raw = data[pos:]
        else:
            raw = data[2:]
        blobs.append(raw)
        want.append(inflate_util.oracle_inflate(raw, 1 << 20))
    laid = _lay(blobs)
    rows = _sizes(inf, blobs, 0, laid=laid)
    dec = _decode(inf, blobs, [1 << 20] * len(blobs), laid=laid)
    for b, (ost, omsg, oout, oused), r, d in zip(blobs, want, rows, dec):
        assert (r[0], r[3]) == (ost, omsg) and _same(r, d) and _starved_count_is_the_oracles(r, (ost, omsg, oout, oused)), (r, d, ost, omsg)
        if ost == 1:
            assert (r[1], r[2]) == (len(oout), oused)


# ---- 2. of the history only its length --------------------------------------------------------------------------------------
def test_history_length_only(mods):
    zr, dfl, inf = mods
    rng = np.random.default_rng(11)
    dic = (b"dictionary words: alpha beta gamma delta epsilon " * 400)[:20000]
    data = dic[5000:9000] + b" and fresh text " + dic[100:3000] + bytes(rng.integers(97, 123, size=5000, dtype=np.uint8))
    s = _raw(data, 9, zdict=dic)
    with pytest.raises(zlib.error):                                              # the stream does reach into the dictionary
        zlib.decompressobj(-15).decompress(s)
    laid = _lay([s, s, s, s])
    rows = _sizes(inf, [s] * 4, 0, dict_len=[len(dic), 0, 32768, len(dic)], laid=laid)
    assert rows[0] == rows[2] == rows[3] == (1, len(data), len(s), "")           # no history byte exists anywhere: none was read
    dec = _decode(inf, [s] * 4, [len(data)] * 4, dict_len=[len(dic), 0, 32768, len(dic)], laid=laid)
    assert dec[1][0] == -3 and dec[1][3] == "invalid distance too far back"
    assert rows[1] == dec[1]                                                     # at the decoder's own count
    assert rows == dec


def test_dictionary_object_zlib_verdicts(mods):
    zr, dfl, inf = mods
    D = (b"shared preset dictionary: lorem ipsum dolor sit amet " * 300)[:9000]
    other = D[:-1] + b"!"
    dic, dic2 = dfl.Dictionary(D), dfl.Dictionary(other)
    plains = [D[100:3000] + b" tail", b"", D[4000:4100] * 3, b"no match here 0123456789" * 20]
    with_d = []
    for p in plains:
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, D)
        with_d.append(c.compress(p) + c.flush())
    clear = [zlib.compress(p, 6) for p in plains]                                # FDICT clear: decoded without history
    blobs = with_d + clear
    want = plains + plains
    laid = _lay(blobs)
    rows = _sizes(inf, blobs, 1, dictionary=dic, laid=laid)
    for b, p, r in zip(blobs, want, rows):
        assert r == (1, len(p), len(b), ""), r
    assert rows == _decode(inf, blobs, [len(p) for p in want], 1, dictionary=dic, laid=laid)
    rows2 = _sizes(inf, blobs, 1, dictionary=dic2, laid=laid)                    # another dictionary: the DICTID mismatch row
    for k, (b, p) in enumerate(zip(blobs, want)):
        assert rows2[k] == ((-3, 0, 6, "") if k < len(plains) else (1, len(p), len(b), "")), (k, rows2[k])
    assert rows2 == _decode(inf, blobs, [len(p) for p in want], 1, dictionary=dic2, laid=laid)
    plain_rows = _sizes(inf, with_d, 1)                                          # no dictionary object: "need dictionary"
    assert all(r == (-3, 0, 0, "need dictionary") for r in plain_rows), plain_rows
    # raw streams made with the dictionary: the object's window counts as present
    raws = [_raw(p, 6, zdict=D) for p in plains]
    assert _sizes(inf, raws, 0, dictionary=dic) == [(1, len(p), len(s), "") for p, s in zip(plains, raws)]
    dic.close()
    dic2.close()


# ---- 3. wrapped members -----------------------------------------------------------------------------------------------------
def _small_pieces():
    mix = synth.silesia_like(300000, seed=5, seg_bytes=64 << 10).tobytes()
    rng = np.random.default_rng(91)
    return [mix[:150000], mix[150000:150000 + 23457], b"", b"a", b"\0" * 100000, rng.integers(0, 256, size=7001, dtype=np.uint8).tobytes(),
            mix[30000:35000], b"abc" * 1111]


def _gzip_members(pieces):
    gz = []
    for k, p in enumerate(pieces):
        buf = io.BytesIO()
        with gzip.GzipFile(filename="name-%d.bin" % k if k % 2 else "", mode="wb", fileobj=buf, compresslevel=6, mtime=1234) as f:
            f.write(p)
        gz.append(buf.getvalue())
    # a hand-made header with FEXTRA + FNAME + FCOMMENT + FHCRC in front of a raw stream
    body = _raw(pieces[1])
    hdr = bytes([0x1f, 0x8b, 8, 4 | 8 | 16 | 2, 1, 2, 3, 4, 0, 3]) + struct.pack("<H", 5) + b"extra" + b"file.txt\0" + b"a comment\0"
    hdr += struct.pack("<H", zlib.crc32(hdr) & 0xffff)
    gz.append(hdr + body + struct.pack("<II", zlib.crc32(pieces[1]), len(pieces[1])))
    return gz, pieces + [pieces[1]]


def test_wrapped_members_of_other_writers(mods):
    zr, dfl, inf = mods
    pieces = _small_pieces()
    zl = [zlib.compress(p, lvl) for p in pieces for lvl in (1, 6, 9)]
    want = [p for p in pieces for _ in range(3)]
    assert _sizes(inf, zl, 1) == [(1, len(p), len(c), "") for p, c in zip(want, zl)]
    gz, want = _gzip_members(pieces)
    gz[0] += b"more bytes"                                                       # bytes behind a complete member are not consumed
    rows = _sizes(inf, gz, 2)
    assert rows == [(1, len(p), len(c) - (10 if k == 0 else 0), "") for k, (p, c) in enumerate(zip(want, gz))]


def test_every_header_refusal_is_the_decoders(mods):
    zr, dfl, inf = mods
    cases = wrapper_cases.cut_and_damaged_members()
    for fmt in (1, 2):
        sel = [c for c in cases if c[0] == fmt]
        assert sel
        laid = _lay([c[1] for c in sel])
        rows = _sizes(inf, [c[1] for c in sel], fmt, laid=laid)
        for c, r in zip(sel, rows):
            assert r == (c[2], 0, 0, c[3]), (fmt, c[1].hex(), r)
        assert rows == _decode(inf, [c[1] for c in sel], [64] * len(sel), fmt, laid=laid)


def test_trailer_presence_and_check_values(mods):
    """a member cut inside its trailer is -5, as in the decode; a wrong check value or ISIZE sizes with status 1 -- there is no
    plaintext to check -- and the packed decode reports it"""
    zr, dfl, inf = mods
    torch = torch_mod()
    p = synth.silesia_like(50000, seed=8).tobytes()
    z, g = zlib.compress(p, 6), gzip.compress(p, 6, mtime=0)

    def mut(b, i, x):
        c = bytearray(b)
        c[i] ^= x
        return bytes(c)

    for fmt, m, tail in ((1, z, 4), (2, g, 8)):
        cuts = [m[:len(m) - k] for k in range(1, tail + 1)]                      # the payload complete, the trailer cut
        rows = _sizes(inf, cuts, fmt)
        assert rows == [(-5, len(p), len(c), STARVED) for c in cuts], rows
        dec = _decode(inf, cuts, [len(p)] * len(cuts), fmt)
        assert [(r[0], r[2], r[3]) for r in rows] == [(d[0], d[2], d[3]) for d in dec]
        bad = [mut(m, len(m) - tail, 0x10)] + ([mut(m, len(m) - 1, 1)] if fmt == 2 else [])
        texts = ["incorrect data check", "incorrect length check"]
        assert _sizes(inf, bad + [m], fmt) == [(1, len(p), len(m), "")] * (len(bad) + 1)
        rows, offs, dst = _packed(inf, bad + [m], fmt, 1, cap=(len(bad) + 1) * len(p))
        assert rows[:len(bad)] == [(-3, len(p), len(m), texts[k]) for k in range(len(bad))], rows
        assert rows[-1] == (1, len(p), len(m), "") and offs == [k * len(p) for k in range(len(bad) + 2)]
        assert dst[len(bad) * len(p):(len(bad) + 1) * len(p)].tobytes() == p and (dst[(len(bad) + 1) * len(p):] == GUARD).all()
        assert rows == _decode(inf, bad + [m], [len(p)] * (len(bad) + 1), fmt)    # the verified rows of the stream call
    del torch


# ---- 4. saturation --------------------------------------------------------------------------------------------------------------
def _run_stream(repeats):
    """BFINAL = 1, BTYPE = 01, the literal 'a', `repeats` x {length 258, distance 1} at 13 bits each, end-of-block (RFC 1951
    3.2.6: 'a' = 0x30 + 97 in 8 bits, length symbol 285 = 0xc5 in 8 bits, distance symbol 0 in 5 bits, codes most significant
    bit first)"""
    def msb(v, n):
        return [(v >> (n - 1 - k)) & 1 for k in range(n)]
    head = np.array([1, 1, 0] + msb(0x30 + 97, 8), dtype=np.uint8)
    pair = np.array(msb(0xc0 + 285 - 280, 8) + [0] * 5, dtype=np.uint8)
    bits = np.concatenate([head, np.tile(pair, repeats), np.zeros(7, dtype=np.uint8)])
    return np.packbits(bits, bitorder="little").tobytes()


def test_saturation_at_the_largest_room(mods):
    zr, dfl, inf = mods
    small = _run_stream(1000)
    assert zlib.decompress(small, -15) == b"a" * 258001                          # the construction itself, against CPython
    repeats = (1 << 31) // 258 + 1
    assert 1 + 258 * repeats > 0x7fffffff >= 1 + 258 * (repeats - 1)
    big = _run_stream(repeats)
    assert 13000000 < len(big) < 14000000
    rows = _sizes(inf, [small, big, small], 0)
    assert rows[0] == rows[2] == (1, 258001, len(small), "")
    assert (rows[1][0], rows[1][1], rows[1][3]) == (-5, 0x7fffffff, FULL) and 0 < rows[1][2] <= len(big), rows[1]


# ---- 5. packed decode -------------------------------------------------------------------------------------------------------
def _packed(inf, blobs, fmt, align, cap=None, dictionary=None, laid=None, extra=4096, stream=None):
    """zng_rocm_uncompress_packed_dev over the blobs into a destination of `cap` bytes (None: ample) inside a tensor filled with
    the guard value -> (rows, offsets, the destination's bytes, `extra` bytes behind dst_cap included)"""
    torch = torch_mod()
    src, offs = laid if laid is not None else _lay(blobs)
    n = len(blobs)
    if cap is None:
        cap = sum(len(zlib.decompressobj({0: -15, 1: 15, 2: 31}[fmt]).decompress(b)) for b in blobs) + 4096 * (n + 1)
    dst = torch.full((cap + extra,), GUARD, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    res = torch.full((max(n, 1), 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    jobs = inf.packed_jobs(src, offs, [len(b) for b in blobs])
    rc = inf.uncompress_packed_dev(fmt, jobs, n, dst[:cap] if cap else None, offsets, res, align, dictionary, stream)
    assert rc == 0, rc
    (stream or torch.cuda.current_stream()).synchronize()
    rows = [(r[2], r[0], r[1], inf.inflate_message(r[3])) for r in res.cpu().tolist()[:n]]
    return rows, offsets.cpu().tolist(), dst.cpu().numpy()


def _expect_layout(sizes, align):
    offs, run = [], 0
    for s in sizes:
        a = max(align, 1)
        run = (run + a - 1) // a * a
        offs.append(run)
        run += s
    return offs + [run]


def _check_layout(dst, offs, plains, cap_end):
    """the plaintexts at their offsets, the guard value in every gap and behind the last byte"""
    pos = 0
    for o, p in zip(offs, plains):
        assert (dst[pos:o] == GUARD).all()
        assert dst[o:o + len(p)].tobytes() == p
        pos = o + len(p)
    assert (dst[pos:] == GUARD).all() and pos <= cap_end


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_packed_decode_of_the_pieces(mods, fmt, align):
    zr, dfl, inf = mods
    import test_gpu_framing_dev as framing
    pieces = framing._pieces()
    blobs = [_raw(p) if fmt == 0 else zlib.compress(p, 6) if fmt == 1 else gzip.compress(p, 6, mtime=0) for p in pieces]
    rows, offs, dst = _packed(inf, blobs, fmt, align)
    assert offs == _expect_layout([len(p) for p in pieces], align)
    assert rows == [(1, len(p), len(b), "") for p, b in zip(pieces, blobs)]
    _check_layout(dst, offs, pieces, offs[-1])


def test_bad_jobs_among_good_ones(mods):
    zr, dfl, inf = mods
    pieces = _small_pieces()
    good = [gzip.compress(p, 6, mtime=0) for p in pieces]
    assert good[0][3] == 0                                                       # no optional field: the payload begins at byte 10
    damaged = good[0][:10] + b"\x07" + good[0][11:]                               # BFINAL, BTYPE = 3: "invalid block type"
    cut = good[1][:len(good[1]) // 2]
    refused = b"\x1e" + good[4][1:]
    blobs = [good[0], damaged, good[1], cut, good[2], refused, good[3], good[5], b"", good[6]]
    kinds = ["ok", "bad", "ok", "bad", "ok", "bad", "ok", "ok", "bad", "ok"]
    plains = [pieces[0], b"", pieces[1], b"", pieces[2], b"", pieces[3], pieces[5], b"", pieces[6]]
    assert plains[4] == b""                                                      # an empty plaintext among the good ones
    laid = _lay(blobs)
    sized = _sizes(inf, blobs, 2, laid=laid)
    ref = _decode(inf, blobs, [len(pieces[0])] * len(blobs), 2, laid=laid)       # the stream call's verdicts on the same members
    for align in (1, 64):
        rows, offs, dst = _packed(inf, blobs, 2, align, cap=sum(len(p) for p in plains) + 64 * len(blobs), laid=laid)
        assert offs == _expect_layout([len(p) for p in plains], align)
        for k, (kind, b, p) in enumerate(zip(kinds, blobs, plains)):
            if kind == "ok":
                assert rows[k] == (1, len(p), len(b), "") == ref[k]
            else:
                assert rows[k] == (sized[k][0], 0, sized[k][2], sized[k][3]), (k, rows[k], sized[k])
                assert (rows[k][0], rows[k][3]) == (ref[k][0], ref[k][3]) and rows[k][0] in (-3, -5)
        _check_layout(dst, offs, plains, offs[-1])
    assert (sized[5][0], sized[5][3]) == (-3, "incorrect header check") and sized[3][0] == -5 and sized[8] == (-5, 0, 0, STARVED)


def test_destination_too_short(mods):
    zr, dfl, inf = mods
    pieces = _small_pieces()
    blobs = [zlib.compress(p, 6) for p in pieces]
    laid = _lay(blobs)
    full = _expect_layout([len(p) for p in pieces], 64)
    k = 4
    end_k = full[k] + len(pieces[k])
    for cap, first_out in ((end_k, k + 1), (end_k - 1, k), (0, 0)):
        rows, offs, dst = _packed(inf, blobs, 1, 64, cap=cap, laid=laid)
        assert offs == full                                                      # the whole layout, d_offsets[njobs] the full need
        for i, (p, b) in enumerate(zip(pieces, blobs)):
            if i < first_out:
                assert rows[i] == (1, len(p), len(b), "") and dst[full[i]:full[i] + len(p)].tobytes() == p
            elif len(p) == 0 and full[i] <= cap:
                # (an empty plaintext ends at its start, so it fits where it starts at or in front of dst_cap: that can only
                # be the job directly behind the last one that fits, and in this batch that job is not empty)
                assert i == first_out and rows[i] == (1, 0, len(b), "")
            else:
                assert rows[i] == (-5, 0, 0, FULL), (cap, i, rows[i])
        # the decoded prefix in place, the guard value in every alignment gap in front of it, between its jobs and behind it:
        # nothing at or behind d_dst + dst_cap, and no padding byte anywhere
        _check_layout(dst, full[:first_out], pieces[:first_out], cap)
    assert pieces[2] == b"" and full[2] > 0                                      # (with dst_cap 0 the empty piece does not fit either)
    rows, offs, dst = _packed(inf, blobs, 1, 64, cap=full[-1], laid=laid, extra=64)   # a second call with that room succeeds
    assert rows == [(1, len(p), len(b), "") for p, b in zip(pieces, blobs)]
    _check_layout(dst, offs, pieces, full[-1])


def test_scan_tiles(mods):
    """4097 streams: past one workgroup's tile of 1024 and no multiple of it; then one stream, then none"""
    zr, dfl, inf = mods
    rng = np.random.default_rng(5)
    words = [b"alpha", b"beta", b"gamma", b"delta", b" ", b"\n", b"0123456789", b"zzzzzzzz"]
    plains = [b"".join(words[int(k)] for k in rng.integers(0, len(words), size=int(rng.integers(0, 5)))) for _ in range(4097)]
    assert min(len(p) for p in plains) == 0 and max(len(p) for p in plains) <= 40
    for n in (4097, 1, 0):
        blobs = [zlib.compress(p, 6) for p in plains[:n]]
        for align in (1, 64) if n == 4097 else (1,):
            rows, offs, dst = _packed(inf, blobs, 1, align, cap=(40 + align) * max(n, 1))
            assert offs == _expect_layout([len(p) for p in plains[:n]], align)
            assert all(a <= b for a, b in zip(offs, offs[1:]))
            assert rows == [(1, len(p), len(b), "") for p, b in zip(plains[:n], blobs)]
            _check_layout(dst, offs, plains[:n], offs[-1])


# ---- 6. the write side's output, read back ------------------------------------------------------------------------------------
def _msgs():
    mix = synth.silesia_like(400000, seed=17, seg_bytes=64 << 10).tobytes()
    rng = np.random.default_rng(23)
    out, pos = [], 0
    for k in range(30):
        n = int(rng.integers(0, 20000)) if k % 7 else (0, 1, 70000, 3)[k // 7 % 4]
        out.append(mix[pos:pos + n])
        pos += n
    return out


def _members(dfl, msgs, fmt, level, dic=None):
    """zng_rocm_compress_members_dev (dic: _dict_dev) over the messages -> (the file on the device, its offsets table there)"""
    torch = torch_mod()
    host = np.frombuffer(b"".join(msgs) + b"\0" * 64, dtype=np.uint8).copy()
    src = torch.from_numpy(host).cuda()
    views, pos = [], 0
    for m in msgs:
        views.append(src[pos:pos + len(m)])
        pos += len(m)
    jobs = dfl.stream_jobs(views)
    n = len(msgs)
    cap = sum(len(m) + len(m) // 8 + 1200 for m in msgs)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    if dic is not None:
        rc = dfl.compress_members_dict_dev(dic, jobs, n, dst, offsets, fmt, level)
    else:
        rc = dfl.compress_members_dev(jobs, n, dst, offsets, fmt, level)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dst, offsets


def _read_back(inf, file_dev, offsets, fmt, total, dic=None):
    """the offsets table as the jobs of the packed call, align 1 -> (rows, offsets, bytes)"""
    torch = torch_mod()
    offs = offsets.cpu().tolist()
    n = len(offs) - 1
    assert offs[-1] <= file_dev.numel()
    jobs = inf.packed_jobs(file_dev, offs[:n], [offs[i + 1] - offs[i] for i in range(n)])
    dst = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    out_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    res = torch.full((n, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    assert inf.uncompress_packed_dev(fmt, jobs, n, dst[:total] if total else None, out_offs, res, 1, dic) == 0
    torch.cuda.synchronize()
    rows = [(r[2], r[0], r[1], inf.inflate_message(r[3])) for r in res.cpu().tolist()]
    return rows, out_offs.cpu().tolist(), dst.cpu().numpy(), offs


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("fmt", [1, 2])
def test_round_trip_with_the_write_side(mods, fmt, level):
    zr, dfl, inf = mods
    msgs = _msgs()
    file_dev, offsets = _members(dfl, msgs, fmt, level)
    whole = b"".join(msgs)
    rows, out_offs, dst, offs = _read_back(inf, file_dev, offsets, fmt, len(whole))
    assert rows == [(1, len(m), offs[i + 1] - offs[i], "") for i, m in enumerate(msgs)]
    assert out_offs == _expect_layout([len(m) for m in msgs], 1)
    assert dst[:len(whole)].tobytes() == whole and (dst[len(whole):] == GUARD).all()


@pytest.mark.parametrize("fmt", [0, 1])
def test_dictionary_form_round_trip(mods, fmt):
    zr, dfl, inf = mods
    msgs = _msgs()
    D = b"".join(msgs[3:9])[-20000:]
    assert len(D) == 20000
    dic = dfl.Dictionary(D)
    file_dev, offsets = _members(dfl, msgs, fmt, 6, dic)
    whole = b"".join(msgs)
    rows, out_offs, dst, offs = _read_back(inf, file_dev, offsets, fmt, len(whole), dic)
    assert rows == [(1, len(m), offs[i + 1] - offs[i], "") for i, m in enumerate(msgs)]
    assert dst[:len(whole)].tobytes() == whole and (dst[len(whole):] == GUARD).all()
    # the members do need the dictionary: CPython reads them with it alone
    host = file_dev.cpu().numpy().tobytes()
    k = max(range(len(msgs)), key=lambda i: len(msgs[i]))
    d = zlib.decompressobj(-15 if fmt == 0 else 15, zdict=D)
    assert d.decompress(host[offs[k]:offs[k + 1]]) == msgs[k]
    dic.close()


# ---- 7. two callers -------------------------------------------------------------------------------------------------------------
def test_two_batches_on_two_streams_from_two_host_threads(mods):
    """the sizing rows and the job table are scratch of the caller's stream: two host threads that run the packed call on
    different batches at the same time must each get their own plaintext, over and over"""
    zr, dfl, inf = mods
    torch = torch_mod()
    each, n = 64 << 10, 96
    work = []
    for k in range(2):
        data = synth.silesia_like(n * each, seed=700 + k, seg_bytes=256 << 10)
        blobs = [zlib.compress(data[i * each:(i + 1) * each].tobytes(), 1 + 5 * k) for i in range(n)]
        src, offs = _lay(blobs)
        work.append(dict(jobs=inf.packed_jobs(src, offs, [len(b) for b in blobs]), src=src, lens=[len(b) for b in blobs],
                         plain=torch.from_numpy(data).cuda(), dst=torch.zeros(n * each, dtype=torch.uint8, device="cuda"),
                         offsets=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                         res=torch.zeros((n, 4), dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            w = work[k]
            s = torch.cuda.Stream()
            for it in range(6):
                w["dst"].zero_()
                w["res"].zero_()
                torch.cuda.current_stream().synchronize()
                rc = inf.uncompress_packed_dev(1, w["jobs"], n, w["dst"], w["offsets"], w["res"], 1, None, s)
                s.synchronize()
                r = w["res"].cpu()
                if rc or not bool((r[:, 2] == 1).all()) or r[:, 1].tolist() != w["lens"] or not torch.equal(w["dst"], w["plain"]) \
                        or w["offsets"].cpu().tolist() != [i * each for i in range(n + 1)]:
                    errors.append((k, it, rc))
                    return
            zr.rocm.lib().zng_rocm_stream_release(s.cuda_stream)
        except Exception as e:                                   # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(mods):
    zr, dfl, inf = mods
    torch = torch_mod()
    EINVAL = -3                                                                  # ZNG_ROCM_EINVAL
    lib = zr.rocm.lib()
    import ctypes as C
    s = zlib.compress(b"some plaintext " * 10)
    src, offs = _lay([s])
    res = torch.full((1, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    offsets = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    dst = torch.full((256,), GUARD, dtype=torch.uint8, device="cuda")
    st = zr.rocm._stream_ptr(None)
    P = zr.rocm._dev_ptr

    def job(**kw):
        jobs = inf.packed_jobs(src, offs, [len(s)])
        for k, v in kw.items():
            setattr(jobs[0], k, v)
        return jobs

    D = dfl.Dictionary(b"dictionary " * 50)
    sizes = [(3, None, job()), (-1, None, job()), (2, D.h, job()), (1, None, job(flags=1)), (1, None, job(in_ptr=None)),
             (1, None, job(in_len=1 << 31)), (0, None, job(dict_len=32769)), (1, None, job(dict_len=5)), (0, D.h, job(dict_len=5))]
    for fmt, d, jobs in sizes:
        assert lib.zng_rocm_inflate_sizes_dev(fmt, d, C.byref(jobs), 1, P(res), st) == EINVAL, fmt
        assert lib.zng_rocm_uncompress_packed_dev(fmt, d, C.byref(jobs), 1, P(dst), 256, 1, P(offsets), P(res), st) == EINVAL, fmt
    assert lib.zng_rocm_inflate_sizes_dev(1, None, C.byref(job()), 1, None, st) == EINVAL
    assert lib.zng_rocm_inflate_sizes_dev(1, None, None, 0, None, st) == 0
    packed = [dict(align=3), dict(align=8192), dict(dst=None), dict(offsets=None), dict(res=None), dict(jobs=job(dict_len=7), fmt=0)]
    for kw in packed:
        a = dict(fmt=1, jobs=job(), dst=P(dst), align=1, offsets=P(offsets), res=P(res))
        a.update(kw)
        assert lib.zng_rocm_uncompress_packed_dev(a["fmt"], None, C.byref(a["jobs"]), 1, a["dst"], 256, a["align"], a["offsets"],
                                                  a["res"], st) == EINVAL, kw
    torch.cuda.synchronize()
    assert (res == 0x5a5a5a5a).all() and (offsets == -1).all() and (dst == GUARD).all()
    D.close()
