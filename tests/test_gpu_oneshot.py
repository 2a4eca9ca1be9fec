"""GPU: compress2 / uncompress2 class front ends -- zlib and gzip framing with on-device trailer checksums.
Cross-checked both ways against CPython's zlib/gzip (independent codec) and the reference's messages."""
import gzip
import hashlib
import importlib
import zlib

import numpy as np
import pytest

import synth
import wrapper_cases
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def one():
    zr = product()
    zr.init()
    return importlib.import_module("zlib-ng_amd.oneshot")


def _data():
    return {
        "mix": synth.silesia_like(2 << 20, seed=5, seg_bytes=512 << 10).tobytes(),
        "empty": b"",
        "short": b"The quick brown fox jumped over the lazy dog",
        "zeros": b"\0" * 700000,
    }


def test_compress2_is_readable_by_python(one):
    torch = torch_mod()
    for name, data in _data().items():
        src = torch.from_numpy(np.frombuffer(data + b"\0" * 16, dtype=np.uint8).copy()).cuda()
        for fmt, level in ((one.ZLIB, -1), (one.ZLIB, 9), (one.GZIP, 6), (one.RAW, 2)):
            dst, clen = one.compress2_dev(src, level=level, fmt=fmt, length=len(data))
            comp = dst[:clen].cpu().numpy().tobytes()
            assert clen <= one.compress_bound(len(data), fmt)
            if fmt == one.ZLIB:
                assert zlib.decompress(comp) == data, name
                assert comp[0] == 0x78 and ((comp[0] << 8) | comp[1]) % 31 == 0
            elif fmt == one.GZIP:
                assert gzip.decompress(comp) == data, name
            else:
                assert zlib.decompressobj(-15).decompress(comp) == data, name


def test_uncompress2_reads_python_streams(one):
    torch = torch_mod()
    for name, data in _data().items():
        dst = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
        for fmt, comp in ((one.ZLIB, zlib.compress(data, 6)), (one.GZIP, gzip.compress(data, 6)),
                          (one.ZLIB, zlib.compress(data, 1) + b"trailing garbage")):
            rc, produced, consumed, msg = one.uncompress2_dev(comp, dst, fmt=fmt)
            assert rc == 0, (name, msg)
            assert produced == len(data) and dst[:produced].cpu().numpy().tobytes() == data
            assert consumed == len(comp) - (16 if comp.endswith(b"trailing garbage") else 0)


def test_uncompress2_errors_use_reference_messages(one):
    """inflate.c:528-543,1127-1147 message texts; uncompr.c:70-75 status mapping"""
    torch = torch_mod()
    data = _data()["mix"][:300000]
    dst = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    z = bytearray(zlib.compress(data, 6))
    g = bytearray(gzip.compress(data, 6))
    bad = bytes(z[:-1]) + bytes([z[-1] ^ 1])
    assert one.uncompress2_dev(bad, dst, fmt=one.ZLIB)[::3] == (-3, "incorrect data check")
    bad = bytes(g[:-5]) + bytes([g[-5] ^ 1]) + bytes(g[-4:])
    assert one.uncompress2_dev(bad, dst, fmt=one.GZIP)[::3] == (-3, "incorrect data check")
    bad = bytes(g[:-1]) + bytes([g[-1] ^ 1])
    assert one.uncompress2_dev(bad, dst, fmt=one.GZIP)[::3] == (-3, "incorrect length check")
    bad = bytes([z[0], z[1] ^ 1]) + bytes(z[2:])
    assert one.uncompress2_dev(bad, dst, fmt=one.ZLIB)[::3] == (-3, "incorrect header check")
    flg = next(f for f in range(32) if ((0x79 << 8) | f) % 31 == 0)
    bad = bytes([0x79, flg]) + bytes(z[2:])            # CM = 9, header check still a multiple of 31
    assert one.uncompress2_dev(bad, dst, fmt=one.ZLIB)[::3] == (-3, "unknown compression method")
    assert one.uncompress2_dev(bytes(z[:len(z) // 2]), dst, fmt=one.ZLIB)[0] == -3      # incomplete stream
    small = torch.zeros(100, dtype=torch.uint8, device="cuda")
    assert one.uncompress2_dev(bytes(z), small, fmt=one.ZLIB)[0] == -5                  # Z_BUF_ERROR
    # the reference's own zlib KAT (test/test_inflate_adler32.cc)
    import json, os
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "inflate_kat.json")))["zlib_stream"]
    rc, produced, consumed, msg = one.uncompress2_dev(bytes.fromhex(kat["hex"]), dst, fmt=one.ZLIB)
    assert rc == 0 and dst[:produced].cpu().numpy().tobytes() == kat["plaintext"].encode()


def test_cut_and_damaged_headers_of_short_members(one):
    """the members of tests/wrapper_cases.py one by one: every one is Z_DATA_ERROR with this call's own text"""
    torch = torch_mod()
    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for fmt, member, _, _, text in wrapper_cases.cut_and_damaged_members():
        rc, _, _, msg = one.uncompress2_dev(member, dst, fmt=fmt)
        assert (rc, msg) == (-3, text), (fmt, member.hex(), rc, msg)


# sha256 of what zng_rocm_compress2_dev writes for wrapper_cases.PLAIN_4K, recorded before the wrapper rules moved to
# framing_parse.h: (format, level)
COMPRESS2_DIGEST = {
    (1, 1): "5d05d5dc979d3b6f86cb94b99ea491fc216aa5bad58c5675298237bc618f09bd",
    (1, 6): "beae34117ab74e470041a2282fdfc52728e41ee7608b359585835e27c40f79a0",
    (1, 9): "907b2e6da6db33e927ec4e789747b3e4e91d27672a22207ecff045e7b44cffec",
    (2, 1): "5c3e07e50e91ea1fca97d03b808b84ac8d9e223c8feef620984720213abed34e",
    (2, 6): "f8c7f033e655a64db654e9d6cd046f26bc5be68c599d7d1bd25321e700042cd2",
    (2, 9): "16069de5c76ffaed1251eb639794f1b50858002ef63633caac643839f08a2a24",
}


def test_compress2_bytes_are_the_recorded_ones(one):
    torch = torch_mod()
    p = wrapper_cases.PLAIN_4K
    src = torch.from_numpy(np.frombuffer(p + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    got = {}
    for (fmt, level) in COMPRESS2_DIGEST:
        dst, clen = one.compress2_dev(src, level=level, fmt=fmt, length=len(p))
        comp = dst[:clen].cpu().numpy().tobytes()
        assert zlib.decompressobj(15 if fmt == 1 else 31).decompress(comp) == p
        got[(fmt, level)] = hashlib.sha256(comp).hexdigest()
        print("compress2_dev", fmt, level, got[(fmt, level)])
    assert got == COMPRESS2_DIGEST


def test_a_large_member_is_inflated_on_the_device(one):
    """uncompress2 / inflate_raw of a member with 4 MiB and more of compressed bytes: up over PCIe once, then
    inflate_large.hip (block starts found on the device, one wavefront per part); trailer checks, too-small destinations
    and damaged streams answer as the sequential decoder does"""
    torch = torch_mod()
    zr = product()
    inf = importlib.import_module("zlib-ng_amd.inflate")
    plain = synth.silesia_like(40 << 20, seed=31).tobytes()
    gz = gzip.compress(plain, 6)
    assert len(gz) > (6 << 20)
    dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    rc, produced, consumed, msg = one.uncompress2_dev(gz, dst, fmt=one.GZIP)
    assert (rc, produced, consumed) == (0, len(plain), len(gz)), (rc, msg)
    assert zr.rocm.lib().zng_rocm_inflate_large_last_parts() >= 32             # decoded in parts on the device
    assert dst[:produced].cpu().numpy().tobytes() == plain
    bad = bytearray(gz)
    bad[-6] ^= 1                                                              # CRC-32 in the trailer
    assert one.uncompress2_dev(bytes(bad), dst, fmt=one.GZIP)[::3] == (-3, "incorrect data check")
    small = torch.zeros(len(plain) - 1, dtype=torch.uint8, device="cuda")
    assert one.uncompress2_dev(gz, small, fmt=one.GZIP)[0] == -5               # Z_BUF_ERROR
    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = raw.compress(plain) + raw.flush()
    rc, produced = inf.inflate_raw(stream[:len(stream) * 3 // 4], dst)         # truncated: the sequential decoder's answer
    assert rc == -5 and zr.rocm.lib().zng_rocm_last_error().decode() == "input ended before the final block"
    rc, produced = inf.inflate_raw(stream, dst)
    assert (rc, produced) == (1, len(plain)) and dst[:produced].cpu().numpy().tobytes() == plain
