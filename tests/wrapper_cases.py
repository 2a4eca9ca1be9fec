"""Short zlib / gzip members that pin what the callers holding a whole member answer to cut and damaged headers
(zng_rocm_uncompress_streams_dev, zng_rocm_uncompress2_dev; the rules: zlib-ng_amd/csrc/framing_parse.h, wrapper_parse_whole),
and the 4 KiB plaintext whose compressed bytes are recorded as digests.  Shared by tests/test_wrapper_whole_cpu.py,
tests/test_gpu_framing_dev.py and tests/test_gpu_oneshot.py."""
import struct
import zlib

PLAIN = b"pack my box with five dozen liquor jugs\n"
PLAIN_4K = b"".join(b"record %05d: the wrapper bytes of every writer stay what they are\n" % i for i in range(80))[:4096]
STARVED = "input ended before the final block"


def gzip_header(extra=None, name=None, comment=None, hcrc=False, mtime=0x04030201, xfl=0, os_=3):
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
    return head


def _raw(plain):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(plain) + c.flush()


def gzip_member(head, plain=PLAIN):
    return head + _raw(plain) + struct.pack("<II", zlib.crc32(plain), len(plain))


ALL_FIELDS = gzip_header(b"extra", b"file name.txt", b"a comment", True)       # FEXTRA FNAME FCOMMENT FHCRC, 43 bytes
MINIMAL = gzip_header()


def cut_and_damaged_members():
    """(format, member, status and text of zng_rocm_uncompress_streams_dev, text of zng_rocm_uncompress2_dev); the one-shot
    call answers every one of them with Z_DATA_ERROR"""
    cases = []
    for n in range(len(ALL_FIELDS)):                                          # the header ends anywhere in front of its end
        cases.append((2, ALL_FIELDS[:n], -5, STARVED, "input ended inside the gzip header"))
    member = gzip_member(ALL_FIELDS)
    wrong = b"\x1e" + member[1:]
    for n in range(2, 10):                                                    # short of ten bytes: starved, whatever they are
        cases.append((2, wrong[:n], -5, STARVED, "input ended inside the gzip header"))
    for n in (10, 11, len(ALL_FIELDS), len(member)):
        cases.append((2, wrong[:n], -3, "incorrect header check", "incorrect header check"))
    for bit in (0x20, 0x40, 0x80):                                            # unknown flag bits
        bad = member[:3] + bytes([member[3] | bit]) + member[4:]
        cases.append((2, bad, -3, "incorrect header check", "unknown header flags set"))
    assert ((0x78 << 8) | 0xbb) % 31 == 0
    for n in range(2, 6):                                                     # FDICT, the DICTID cut short
        cases.append((1, (b"\x78\xbb" + b"\x01\x02\x03")[:n], -3, "need dictionary", "preset dictionary required"))
    return cases
