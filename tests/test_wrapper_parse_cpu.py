"""zng_rocm_wrapper_parse on a machine without a device: the zlib (RFC 1950) and gzip (RFC 1952) header rules that the
header kernel of the wrapped large calls runs too (zlib-ng_amd/csrc/framing_parse.h, one function for host and device;
inflate.c:509-555, :556-700, :702-715).  Oracle: CPython's zlib -- decompressobj(15) / decompressobj(31) on the whole member
for what a header is answered with, decompressobj(-15) on the bytes behind header_len for where the payload begins."""
import glob
import gzip
import importlib
import io
import itertools
import os
import struct
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TEXTS = ("incorrect header check", "unknown compression method", "invalid window size", "unknown header flags set",
                "header crc mismatch")
PLAIN = b"".join(b"line %d of the wrapper test: pack my box with five dozen liquor jugs\n" % i for i in range(400))
DICT = PLAIN[:1000]


@pytest.fixture(scope="module")
def parse():
    """never initialises the device: the function must work before zng_rocm_init"""
    importlib.import_module("zlib-ng_amd")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    return inf.wrapper_parse


def _raw(plain, zdict=None):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zdict) if zdict else zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(plain) + c.flush()


def _gzip_member(plain, extra=None, name=None, comment=None, hcrc=False, mtime=0x12345678, xfl=2, os_=3):
    flags = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    head = bytes([0x1f, 0x8b, 8, flags]) + struct.pack("<IBB", mtime, xfl, os_)
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head, _raw(plain), struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)


def _cpython(fmt, member, zdict=None):
    """what CPython says to the whole member: ("ok", plaintext, unused) or ("error", text)"""
    wbits = 15 if fmt == 1 else 31
    d = zlib.decompressobj(wbits, zdict) if zdict is not None else zlib.decompressobj(wbits)
    try:
        out = d.decompress(member)
    except zlib.error as e:
        return "error", str(e)
    return ("ok", out, d.unused_data) if d.eof else ("short", out, b"")


def _payload_is_at(member, header_len, plain, trailer_and_behind, zdict=None):
    d = zlib.decompressobj(-15, zdict) if zdict is not None else zlib.decompressobj(-15)
    assert d.decompress(member[header_len:]) == plain and d.eof
    assert d.unused_data == trailer_and_behind


def test_zlib_headers_every_level_hint_and_window(parse):
    raw = _raw(PLAIN)
    trailer = struct.pack(">I", zlib.adler32(PLAIN))
    for wbits in range(8, 16):
        for flevel in range(4):
            cmf = 8 | ((wbits - 8) << 4)
            flg = flevel << 6
            flg += 31 - ((cmf << 8) | flg) % 31
            member = bytes([cmf, flg & 0xff]) + raw + trailer + b"behind"
            assert _cpython(1, member)[0] == "ok"
            assert parse(1, member) == (0, 2, 0, 0, None), (wbits, flevel)
            _payload_is_at(member, 2, PLAIN, trailer + b"behind")
    for level in (1, 6, 9):
        member = zlib.compress(PLAIN, level)
        assert parse(1, member) == (0, 2, 0, 0, None)


def test_zlib_header_with_fdict(parse):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, DICT)
    member = c.compress(PLAIN) + c.flush()
    assert member[1] & 0x20
    st, hl, dictid, fdict, msg = parse(1, member)
    assert (st, hl, dictid, fdict, msg) == (2, 6, zlib.adler32(DICT), 1, None)
    assert _cpython(1, member)[0] == "error" and "Error 2" in _cpython(1, member)[1]
    assert _cpython(1, member, DICT)[:2] == ("ok", PLAIN)
    _payload_is_at(member + b"xy", hl, PLAIN, member[-4:] + b"xy", zdict=DICT)
    for cut in range(6):
        assert parse(1, member[:cut])[0] == -5, cut


def test_gzip_headers_every_combination_of_optional_fields(parse):
    minimal = gzip.compress(PLAIN)
    st, hl, dictid, fdict, msg = parse(2, minimal)
    assert (st, hl, dictid, fdict, msg) == (0, 10, 0, 0, None)
    _payload_is_at(minimal, 10, PLAIN, minimal[-8:])
    buf = io.BytesIO()
    with gzip.GzipFile("a name.txt", "wb", fileobj=buf) as f:
        f.write(PLAIN)
    named = buf.getvalue()
    assert parse(2, named)[:2] == (0, 10 + len(b"a name.txt") + 1)
    rng_extra = bytes((i * 37 + 11) & 0xff for i in range(65535))        # zeros inside: FEXTRA is counted, not searched
    for extra, name, comment, hcrc in itertools.product((None, b"", rng_extra[:5], rng_extra), (None, b"shard-00017.bin"),
                                                        (None, b"", b"a comment"), (False, True)):
        head, raw, trailer = _gzip_member(PLAIN, extra, name, comment, hcrc)
        member = head + raw + trailer + b"next"
        got = _cpython(2, member)
        assert got == ("ok", PLAIN, b"next"), (extra and len(extra), name, comment, hcrc)
        assert parse(2, member) == (0, len(head), 0, 0, None), (extra and len(extra), name, comment, hcrc)
        _payload_is_at(member, len(head), PLAIN, trailer + b"next")
        if extra is None or len(extra) <= 5:
            for cut in range(len(head)):                                  # every truncation inside the header
                assert parse(2, member[:cut])[0] == -5, (cut, len(head))
        else:
            for cut in list(range(16)) + [len(head) // 2, len(head) - 3, len(head) - 1]:
                assert parse(2, member[:cut])[0] == -5, (cut, len(head))
        assert parse(2, member[:len(head)])[:2] == (0, len(head))         # complete header, empty payload: accepted


def test_committed_reference_fixtures(parse):
    """the .gz / zlib members under tests/golden/ref_fixtures: CPython on the whole file and on the payload behind header_len
    say the same"""
    seen = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "*"))):
        data = open(path, "rb").read()
        for fmt in (1, 2):
            if fmt == 2 and not path.endswith(".gz"):
                continue
            whole = _cpython(fmt, data)
            st, hl, dictid, fdict, msg = parse(fmt, data)
            if whole[0] == "error" and any(t in whole[1] for t in HEADER_TEXTS):
                assert st == -3 and msg in whole[1], (path, fmt, whole, st, msg)
                continue
            if fmt == 1 and path.endswith(".gz"):
                continue
            assert st == 0, (path, fmt, st, msg)
            seen += 1
            d = zlib.decompressobj(-15)
            try:
                out = d.decompress(data[hl:])
                behind = ("ok", out, d.unused_data[4 if fmt == 1 else 8:]) if d.eof else ("short", out, b"")
            except zlib.error as e:
                behind = ("error", str(e))
            if whole[0] == "error" and ("data check" in whole[1] or "length check" in whole[1]):
                assert behind[0] == "ok", (path, whole, behind[0])        # the payload is whole, the trailer is wrong
            else:
                assert behind == whole, (path, fmt, whole[0], behind[0])
    assert seen >= 5


def _judge_mutation(parse, fmt, member, what):
    got = _cpython(fmt, member)
    st, hl, dictid, fdict, msg = parse(fmt, member)
    if got[0] == "error" and any(t in got[1] for t in HEADER_TEXTS):
        assert st == -3 and msg is not None and msg in got[1], (what, got[1], st, msg)
    elif got[0] == "error" and "Error 2 " in got[1]:                      # Z_NEED_DICT
        assert (st, hl, fdict) == (2, 6, 1) and dictid == struct.unpack(">I", member[2:6])[0], (what, st, hl, dictid)
    else:
        assert st in (0, -5), (what, got[0], st, msg)
    return st, hl


def test_every_single_byte_mutation_of_the_first_four_bytes(parse):
    zmember = zlib.compress(PLAIN, 6)
    head, raw, trailer = _gzip_member(PLAIN, None, b"name", None, True)
    gmember = head + raw + trailer
    assert parse(2, gmember) == (0, len(head), 0, 0, None)
    for fmt, member in ((1, zmember), (2, gmember)):
        for at in range(4):
            for value in range(256):
                if value == member[at]:
                    continue
                mutated = bytearray(member)
                mutated[at] = value
                _judge_mutation(parse, fmt, bytes(mutated), (fmt, at, value))
    # MTIME, XFL, OS: any value, the header keeps its length (no FHCRC here: it would cover them)
    head, raw, trailer = _gzip_member(PLAIN, None, b"name", None, False)
    plainmember = head + raw + trailer
    for at in range(4, 10):
        for value in (0, 1, 0x7f, 0x80, 0xff):
            mutated = bytearray(plainmember)
            mutated[at] = value
            assert _cpython(2, bytes(mutated))[0] == "ok"
            assert parse(2, bytes(mutated)) == (0, len(head), 0, 0, None), (at, value)
    # a wrong FHCRC, and a header byte changed under a right one
    head, raw, trailer = _gzip_member(PLAIN, b"\x01\x02\x03\x04\x05", b"name", b"comment", True)
    for at, flip in ((len(head) - 1, 0x01), (len(head) - 2, 0x80), (5, 0x10), (12, 0x01)):
        mutated = bytearray(head + raw + trailer)
        mutated[at] ^= flip
        got = _cpython(2, bytes(mutated))
        assert got[0] == "error" and "header crc mismatch" in got[1]
        assert parse(2, bytes(mutated)) == (-3, 0, 0, 0, "header crc mismatch"), at


def test_gzip_magic_and_formats(parse):
    member = gzip.compress(PLAIN)
    assert parse(2, zlib.compress(PLAIN)) == (-3, 0, 0, 0, "incorrect header check")     # a zlib member is no gzip member
    assert parse(2, b"\x1f\x8c" + member[2:])[4] == "incorrect header check"
    assert parse(2, b"\x1f\x8b\x07")[0] == -5 and parse(2, b"\x1f\x8b\x07\x00")[4] == "unknown compression method"
    assert parse(2, b"\x1f\x8b\x08\x20")[4] == "unknown header flags set"
    assert parse(0, member) == (0, 0, 0, 0, None)
    for fmt in (-1, 3, 47):
        assert parse(fmt, member) == (-3, 0, 0, 0, None)                                  # ZNG_ROCM_EINVAL, no text
    assert parse(1, b"") == (-5, 0, 0, 0, None) and parse(2, b"") == (-5, 0, 0, 0, None)


def test_runs_without_a_device(parse):
    zr = importlib.import_module("zlib-ng_amd")
    if zr.device_count() == 0:
        assert not zr.available()
    assert parse(2, gzip.compress(b"x"))[:2] == (0, 10)
