"""What the gzip header tests share: a model of the header deflate.c:923-1020 writes, made here with struct and zlib.crc32 and
never with the code under test, and the field sets the CPU and GPU tests render."""
import struct
import zlib


def want_xfl(level, strategy):
    level = 6 if level == -1 else level
    return 2 if level == 9 else 4 if (strategy >= 2 or level < 2) else 0


def model_header(level=6, strategy=0, time=0, os=3, text=False, hcrc=False, extra=None, name=None, comment=None):
    """RFC 1952 2.3: ID1 ID2 CM FLG MTIME XFL OS [XLEN extra] [name 0] [comment 0] [CRC16]; None = the field is absent"""
    flg = (1 if text else 0) | (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0) | \
        (16 if comment is not None else 0)
    out = struct.pack("<BBBBIBB", 0x1f, 0x8b, 8, flg, time & 0xffffffff, want_xfl(level, strategy), os & 0xff)
    if extra is not None:
        out += struct.pack("<H", len(extra)) + extra
    if name is not None:
        out += name + b"\0"
    if comment is not None:
        out += comment + b"\0"
    if hcrc:
        out += struct.pack("<H", zlib.crc32(out) & 0xffff)
    return out


def fields(flg, size=1, seed=0):
    """keyword arguments of model_header / GzipHeader.make for the five flag bits `flg`; size 0: empty fields, 1: small ones"""
    kw = {"time": (0x5f000000 + 977 * seed + flg) & 0xffffffff, "os": (3, 0, 255, 0x1ff)[(flg + seed) % 4], "text": bool(flg & 1),
          "hcrc": bool(flg & 2)}
    if flg & 4:
        kw["extra"] = b"" if size == 0 else b"Ap\x03\x00" + bytes([seed & 0xff, 0, 0xfe])
    if flg & 8:
        kw["name"] = b"" if size == 0 else b"member-%d.txt" % seed
    if flg & 16:
        kw["comment"] = b"" if size == 0 else b"written by test %d" % seed
    return kw


def padded(total, flg=8 | 16 | 2, seed=0):
    """fields whose header is exactly `total` bytes: a name and a comment that share what is left, none of them with a zero byte"""
    kw = fields(flg & ~4, 0, seed)
    fixed = 10 + (2 if flg & 2 else 0) + (1 if flg & 8 else 0) + (1 if flg & 16 else 0)
    left = total - fixed
    assert left >= 0 and flg & 24
    pat = bytes(range(1, 256)) * (left // 255 + 1)
    if flg & 8 and flg & 16:
        kw["name"], kw["comment"] = pat[:left // 2], pat[7:7 + left - left // 2]
    elif flg & 8:
        kw["name"] = pat[:left]
    else:
        kw["comment"] = pat[:left]
    assert len(model_header(**kw)) == total
    return kw


def biggest(seed=0):
    """the 196621 bytes a header can have"""
    kw = fields(31, 1, seed)
    pat = bytes(range(1, 256)) * 258
    kw["extra"], kw["name"], kw["comment"] = bytes(range(256)) * 255 + bytes(255), pat[:65535], pat[3:65538]
    assert len(model_header(**kw)) == 196621
    return kw


def make_head(dfl, kw):
    """the GzipHeader (zlib-ng_amd.deflate) of model_header's keyword arguments"""
    return dfl.GzipHeader.make(**{k: v for k, v in kw.items() if k not in ("level", "strategy")})


def gzip_member(head, plain, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return head + c.compress(plain) + c.flush() + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)
