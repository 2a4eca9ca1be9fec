"""Multi-member gzip files for the tests of zng_rocm_gunzip_members_dev and tools/gunzip_members_rate.py: hand-made BGZF blocks
(SAM specification 4.1: an 18-byte header with the 'BC' subfield, raw deflate of at most 65280 bytes of plaintext, CRC-32 and
ISIZE; the 28-byte end-of-file block), the regular expression that restates the scan rule, and the oracle -- a loop of
zlib.decompressobj(31) over unused_data, which is how CPython (and gzread) reads such a file."""
import re
import struct
import zlib

from wrapped_members import raw, trailer

SCAN = re.compile(rb"(?=\x1f\x8b\x08[\x00-\x1f])", re.S)
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZF_BLOCK = 65280


def bgzf_block(plain, level=6, extra_front=b"", extra_behind=b""):
    """one BGZF member: the 'BC' subfield carries BSIZE = total bytes - 1"""
    assert len(plain) <= BGZF_BLOCK
    data = raw(plain, level)
    xlen = len(extra_front) + 6 + len(extra_behind)
    total = 12 + xlen + len(data) + 8
    assert total <= 65536
    head = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + extra_front + b"BC" + struct.pack("<HH", 2, total - 1) + \
        extra_behind
    return head + data + trailer(2, plain)


def bgzf_file(plain, level=6, block=BGZF_BLOCK):
    return b"".join(bgzf_block(plain[at:at + block], level) for at in range(0, len(plain), block)) + BGZF_EOF


def scan(data):
    return [m.start() for m in SCAN.finditer(data)]


def has_bc(member):
    """does the header carry a 'BC' subfield with SLEN 2?  (RFC 1952 2.3.1.1, walked independently of the library)"""
    if len(member) < 12 or not member[3] & 4:
        return 0
    xlen, = struct.unpack_from("<H", member, 10)
    field, at = member[12:12 + xlen], 0
    if len(field) < xlen:
        return 0
    while at + 4 <= len(field):
        slen, = struct.unpack_from("<H", field, at + 2)
        if at + 4 + slen > len(field):
            return 0
        if field[at:at + 2] == b"BC" and slen == 2:
            return 1
        at += 4 + slen
    return 0


def oracle_members(data):
    """([(src_off, src_len, plaintext)], end of the last member): the members CPython reads; a member in trouble raises"""
    out, at = [], 0
    while not out or (len(data) - at >= 2 and data[at:at + 2] == b"\x1f\x8b"):
        d = zlib.decompressobj(31)
        plain = d.decompress(data[at:])
        if not d.eof:
            raise zlib.error("incomplete member at %d" % at)
        used = len(data) - at - len(d.unused_data)
        out.append((at, used, plain))
        at += used
    return out, at


def oracle_table(data):
    """the rows of zng_rocm_gzip_member the call must report: (src_off, src_len, dst_off, out_len, crc, bgzf)"""
    members, end = oracle_members(data)
    rows, dst = [], 0
    for off, used, plain in members:
        rows.append((off, used, dst, len(plain), zlib.crc32(plain), has_bc(data[off:off + used])))
        dst += len(plain)
    return rows, b"".join(m[2] for m in members), end


def zero_free_stored_member(pattern, blocks):
    """a valid gzip member of `blocks` stored blocks whose deflate data holds no zero byte: every block is 0x7f7f bytes of
    `pattern` repeated (LEN 7f 7f, NLEN 80 80) behind a block header whose five padding bits are ones (f8, the last one f9).
    With pattern 1f 8b 08 08 every fourth byte begins a candidate with FNAME set and no zero byte up to the trailer."""
    assert b"\x00" not in pattern
    plain = (pattern * (0x7f7f * blocks // len(pattern) + 1))[:0x7f7f * blocks]
    body = b"".join(bytes([0xf9 if k == blocks - 1 else 0xf8]) + b"\x7f\x7f\x80\x80" + plain[k * 0x7f7f:(k + 1) * 0x7f7f]
                    for k in range(blocks))
    assert b"\x00" not in body
    member = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + body + struct.pack("<II", zlib.crc32(plain), len(plain))
    assert zlib.decompressobj(31).decompress(member) == plain
    return member, plain
