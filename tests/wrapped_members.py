"""Wrapped members for the large device inflaters: the zlib / gzip writers, the device placement at odd addresses and the
mixed batch that tests/test_gpu_uncompress_large.py checks and tools/uncompress_large_rate.py times."""
import gzip
import io
import struct
import zlib

import numpy as np

import synth

MiB = 1 << 20
SUB = MiB // 2                                            # the check pass's sub-message (framing_large.hip kSubBytes)
ODDS = (1, 3, 7, 9, 5, 11, 15, 13)


def place(torch, data, odd):
    """the bytes in device memory at an address that is `odd` modulo 16"""
    n = len(data)
    buf = torch.zeros(odd + n + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if n:
        buf[odd:odd + n] = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()
    return buf[odd:odd + n]


def plain(mib, k, extra=0):
    return synth.silesia_like(mib * MiB + extra, seed=0x6A21 + k).tobytes()


def raw(plain, level=6, zdict=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zdict) if zdict else \
        zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(plain) + c.flush()


def trailer(fmt, plain):
    return struct.pack(">I", zlib.adler32(plain)) if fmt == 1 else struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)


def gzip_file(plain, name, level=6):
    buf = io.BytesIO()
    with gzip.GzipFile(name, "wb", compresslevel=level, fileobj=buf, mtime=1700000000) as f:
        f.write(plain)
    return buf.getvalue()


def handmade(plain, level=6, name=b"file.txt", hcrc=True):
    """FEXTRA + FNAME + FCOMMENT + FHCRC in front of a raw stream"""
    head = bytes([0x1f, 0x8b, 8, 4 | 8 | 16 | (2 if hcrc else 0), 1, 2, 3, 4, 0, 3]) + struct.pack("<H", 5) + b"extra" + name + b"\0" + \
        b"a comment\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + raw(plain, level) + trailer(2, plain)


def wrap(fmt, plain, level=6):
    return zlib.compress(plain, level) if fmt == 1 else gzip_file(plain, "", level)


def own_compress2(torch, one, fmt, plain):
    src = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
    dst, n = one.compress2_dev(src, level=6, fmt=fmt)
    return dst[:n].cpu().numpy().tobytes()


def own_wrapped_quick(torch, dfl, fmt, plain):
    n = len(plain)
    src = torch.zeros((n + 15) & ~15, dtype=torch.uint8, device="cuda")
    src[:n] = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
    w = dfl.WrappedBatch(src, [0], [n], fmt)
    w.run()
    torch.cuda.synchronize()
    return w.compressed(0)


class Member:
    """one job: the member's bytes (possibly with bytes behind), the plaintext a clean decode gives (or None), an optional
    dictionary, dst_cap; `first` = length of the first member"""

    def __init__(self, torch, name, data, plain, odd, first=None, zdict=None, cap=None):
        self.name, self.data, self.plain, self.odd = name, bytes(data), plain, odd
        self.first = len(self.data) if first is None else first
        self.src = place(torch, self.data, odd)
        self.zdict = None if zdict is None else place(torch, zdict, (odd + 4) % 16)
        self.cap = (len(plain) if plain is not None else 8 * MiB) if cap is None else cap

    def dst(self, torch, guard=64):
        whole = torch.full((16 + self.cap + guard,), 0xAB, dtype=torch.uint8, device="cuda")
        assert whole.data_ptr() % 16 == 0
        return whole, whole[self.odd:self.odd + self.cap]


def mixed(torch, dfl, one, fmt):
    k = iter(range(100))
    odd = lambda: ODDS[next(k) % 8]                                          # noqa: E731
    ms = []

    def add(name, data, plain, first=None):
        ms.append(Member(torch, name, data, plain, odd(), first=first))

    if fmt == 1:
        for name, mib, level in (("zlib1-8", 8, 1), ("zlib6-32", 32, 6), ("zlib9-4", 4, 9), ("zlib6-2", 2, 6), ("zlib6-5", 5, 6),
                                 ("zlib1-3", 3, 1)):
            p = plain(mib, len(ms), extra=977 * len(ms))
            add(name, zlib.compress(p, level), p)
    else:
        for name, mib, fname in (("gzfile-8", 8, ""), ("gzfile-named-32", 32, "shard-00017.bin"), ("gzfile-named-2", 2, "a b.txt")):
            p = plain(mib, len(ms), extra=977 * len(ms))
            add(name, gzip_file(p, fname), p)
        for name, mib, level in (("handmade-4", 4, 9), ("handmade-5", 5, 6), ("handmade-3", 3, 1)):
            p = plain(mib, len(ms), extra=977 * len(ms))
            add(name, handmade(p, level), p)
    for name, mib in (("own-compress2-16", 16), ("own-compress2-2", 2)):
        p = plain(mib, len(ms), extra=31 * len(ms))
        add(name, own_compress2(torch, one, fmt, p), p)
    for name, mib in (("own-quick-4", 4), ("own-quick-8", 8)):
        p = plain(mib, len(ms))
        add(name, own_wrapped_quick(torch, dfl, fmt, p), p)
    p = plain(4, len(ms), extra=5)
    c = wrap(fmt, p)
    add("garbage-behind", c + bytes(range(1, 101)), p, first=len(c))
    p = plain(6, len(ms), extra=1)
    c = wrap(fmt, p)
    add("second-member-behind", c + wrap(fmt, b"the second member " * 1000), p, first=len(c))
    assert len(ms) >= 12
    for name, n in (("empty", 0), ("one-byte", 1), ("sub-1", SUB - 1), ("sub", SUB), ("sub+1", SUB + 1)):
        p = bytes([0x41 + len(name)]) * n
        add("run-" + name, wrap(fmt, p), p)
    return ms
