"""zng_rocm_gunzip_members_dev: every member of a gzip file that sits in device memory, BGZF included -- what gzread does with a
file of several members (gz_look gzread.c.in:81-154, gz_decomp :161-207) in place of the caller's loop over
zng_rocm_uncompress_large_dev(2, ...).  Through the C ABI, file and plaintext at odd device addresses, 0xAB around the
plaintext.  Oracles: the plaintext, and a Python loop of zlib.decompressobj(31) over unused_data for the members' boundaries
and CRC-32s (gzip_files.oracle_table); for the first member and for single-member files, zng_rocm_uncompress_large_dev itself."""
import ctypes as C
import importlib
import struct
import zlib

import pytest

import synth
from gzip_files import BGZF_BLOCK, BGZF_EOF, bgzf_block, bgzf_file, oracle_table, scan, zero_free_stored_member
from wrapped_members import MiB, gzip_file, handmade, own_compress2, place

pytestmark = pytest.mark.gpu
KiB = 1 << 10


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), importlib.import_module("zlib-ng_amd.oneshot"), zr


def _plain(n, seed):
    return synth.silesia_like(n, seed=0x6B00 + seed).tobytes() if n else b""


def _error(zr):
    return zr.rocm.lib().zng_rocm_last_error().decode()


class Run:
    """one call: the file at an address that is `odd` modulo 16, the plaintext at another odd address inside 0xAB"""

    def __init__(self, mods, data, cap, odd=3, **kw):
        torch, inf, _, zr = mods
        self.src = place(torch, data, odd)
        self.odd, self.cap = (odd + 6) % 16 | 1, cap
        self.whole = torch.full((16 + cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.dst = self.whole[self.odd:self.odd + cap]
        torch.cuda.synchronize()
        self.status, self.out_len, self.in_used, self.rows, self.nmembers, self.counters = inf.gunzip_members_dev(self.src, self.dst, **kw)
        torch.cuda.synchronize()
        self.error = _error(zr)
        # nothing in front of the plaintext, nothing at or behind d_dst + dst_cap
        assert int(self.whole[:self.odd].min()) == 0xAB and int(self.whole[self.odd + cap:].min()) == 0xAB

    def plain(self):
        return self.dst[:self.out_len].cpu().numpy().tobytes()

    def untouched(self):
        return int(self.whole.min()) == 0xAB


def _check_whole_file(r, data, note):
    rows, plain, end = oracle_table(data)
    assert (r.status, r.out_len, r.in_used, r.nmembers) == (1, len(plain), end, len(rows)), (note, r.status, r.out_len, r.in_used, r.error)
    assert r.rows == rows, note
    assert r.plain() == plain, note
    return rows


# ---- BGZF -------------------------------------------------------------------------------------------------------------------
def test_bgzf_64_mib(mods):
    plain = _plain(64 * MiB + 12345, 1)
    data = bgzf_file(plain)
    assert data.endswith(BGZF_EOF) and len(BGZF_EOF) == 28 and data[:4] == b"\x1f\x8b\x08\x04" and data[12:16] == b"BC\x02\x00"
    r = Run(mods, data, len(plain))
    rows = _check_whole_file(r, data, "bgzf")
    assert len(rows) == -(-len(plain) // BGZF_BLOCK) + 1 and all(row[5] == 1 for row in rows)
    assert rows[-1][1:4] == (28, len(plain), 0)                          # the EOF block is a member
    assert r.counters == {"candidates": len(scan(data)), "replans": 0, "small": len(rows), "large": 0}, r.counters


# ---- concatenated members of mixed size and writer ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_file(mods):
    torch, _, one, _ = mods
    gz, own = (lambda p: gzip_file(p, "shard.bin")), (lambda p: own_compress2(torch, one, 2, p))
    order = ((0, gz), (1, handmade), (100 * KiB, own), (3 * MiB, gz), (40 * MiB, handmade), (1, own), (100 * KiB, gz), (3 * MiB, handmade),
             (0, handmade), (3 * MiB, own), (100 * KiB, handmade), (1, gz))
    return b"".join(writer(_plain(size, 10 + k)) for k, (size, writer) in enumerate(order))


@pytest.mark.parametrize("subblock", [False, True])
def test_concatenated_members_of_mixed_size(mods, mixed_file, subblock):
    data = mixed_file
    rows, plain, end = oracle_table(data)
    assert end == len(data) and len(rows) == 12
    assert {row[3] for row in rows} >= {0, 1, 100 * KiB, 3 * MiB, 40 * MiB}
    r = Run(mods, data, len(plain), odd=7, subblock=subblock)
    _check_whole_file(r, data, "mixed")
    hits = scan(data)
    inside = [p for p in hits if any(off < p < off + used for off, used, _, _, _, _ in rows)]
    assert r.counters["candidates"] == len(hits)
    assert r.counters["small"] > 0 and r.counters["large"] > 0 and r.counters["small"] + r.counters["large"] == len(rows), r.counters
    assert r.counters["replans"] <= len(inside), (r.counters, inside)


# ---- a valid member inside a stored block ------------------------------------------------------------------------------------
def test_a_member_inside_a_stored_block(mods):
    inner = gzip_file(_plain(40 * KiB, 30), "inner.txt")                 # a complete valid gzip file ...
    assert zlib.decompressobj(31).decompress(inner) and len(inner) < BGZF_BLOCK
    outer = gzip_file(inner, "", 0)                                      # ... is the plaintext of a level-0 member
    assert outer.find(inner) > 0
    two = [gzip_file(_plain(300 * KiB, 31), "second.txt"), handmade(_plain(50 * KiB, 32))]
    # 1. followed by two ordinary members: the inner member's header is the next candidate, with nothing to say otherwise
    data = outer + two[0] + two[1]
    r = Run(mods, data, len(inner) + 350 * KiB)
    rows = _check_whole_file(r, data, "nested, then two")
    assert len(rows) == 3 and all(row[0] != outer.find(inner) for row in r.rows) and r.rows[0][3] == len(inner)
    assert r.counters["replans"] >= 1 and r.counters["candidates"] >= 4, r.counters
    # 2. the same with the guess far enough inside that only decoding refutes it
    # (the eight bytes in front of the inner member read as a CRC-32 and an ISIZE of 700: a guess that could be right)
    front = b"in front of the inner member: " * 40 + struct.pack("<II", 0x12345678, 700)
    data = gzip_file(front + inner, "", 0) + two[0] + two[1]
    r = Run(mods, data, len(front) + len(inner) + 350 * KiB, odd=9)
    rows = _check_whole_file(r, data, "nested behind text, then two")
    assert len(rows) == 3 and r.counters["replans"] >= 1, r.counters
    # 3. as a BGZF block: BSIZE hops over it
    data = bgzf_block(inner, level=0) + bgzf_block(_plain(60000, 33)) + BGZF_EOF
    r = Run(mods, data, len(inner) + 60000, odd=5)
    rows = _check_whole_file(r, data, "nested in a BGZF block")
    assert len(rows) == 3 and r.counters["replans"] == 0 and r.counters["large"] == 0, r.counters
    assert r.counters["candidates"] == len(scan(data)) >= 4, r.counters


# ---- trouble ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three():
    plains = [_plain(200 * KiB, 40), _plain(3 * MiB + 5, 41), _plain(70 * KiB, 42)]
    return plains, [gzip_file(plains[0], "one"), handmade(plains[1]), gzip_file(plains[2], "")]


def test_trailing_garbage_and_one_trailing_1f(mods, three):
    plains, members = three
    whole = b"".join(members)
    for behind in (b"\x00" * 100, bytes(range(1, 200)), b"\x1f", b"\x1f\x8c" + b"x" * 50, b"\x8b\x1f"):
        r = Run(mods, whole + behind, sum(map(len, plains)))
        assert (r.status, r.in_used, r.nmembers, r.out_len) == (1, len(whole), 3, sum(map(len, plains))), (behind[:4], r.status, r.error)
        assert r.plain() == b"".join(plains) and r.rows == oracle_table(whole)[0]


def test_second_member_with_a_wrong_crc(mods, three):
    plains, members = three
    bad = bytearray(members[1])
    bad[-8] ^= 0x01
    with pytest.raises(zlib.error, match="incorrect data check"):
        zlib.decompressobj(31).decompress(bytes(bad))
    r = Run(mods, members[0] + bytes(bad) + members[2], sum(map(len, plains)))
    assert (r.status, r.error, r.nmembers) == (-3, "incorrect data check", 1), (r.status, r.error)
    assert r.out_len == len(plains[0]) + len(plains[1]) and r.rows == oracle_table(members[0])[0]
    assert r.dst[:len(plains[0])].cpu().numpy().tobytes() == plains[0]
    bad = bytearray(members[1])
    bad[-1] ^= 0x01
    r = Run(mods, members[0] + bytes(bad) + members[2], sum(map(len, plains)))
    assert (r.status, r.error, r.nmembers) == (-3, "incorrect length check", 1), (r.status, r.error)


def test_second_member_truncated_in_its_last_16_bytes(mods, three):
    plains, members = three
    for second in (members[2], members[1]):                              # a member of each engine
        for cut in range(1, 17):
            data = members[0] + second[:-cut]
            r = Run(mods, data, sum(map(len, plains)), odd=1 + 2 * (cut % 8))
            assert (r.status, r.nmembers) == (-5, 1), (cut, r.status, r.error)
            assert r.in_used <= len(data) and r.out_len >= len(plains[0]) and r.rows == oracle_table(members[0])[0], cut
            if cut <= 8:                                                 # cut inside the trailer: the plaintext is complete
                assert r.in_used == len(data), (cut, r.in_used)


def test_third_member_with_method_7_and_other_header_trouble(mods, three):
    plains, members = three
    front = members[0] + members[1]
    for third, text in ((members[2][:2] + b"\x07" + members[2][3:], "unknown compression method"),
                        (members[2][:3] + bytes([members[2][3] | 0x40]) + members[2][4:], "unknown header flags set")):
        with pytest.raises(zlib.error, match=text):
            zlib.decompressobj(31).decompress(third)
        r = Run(mods, front + third, sum(map(len, plains)))
        assert (r.status, r.error, r.nmembers, r.in_used) == (-3, text, 2, len(front)), (r.status, r.error, r.in_used)
        assert r.out_len == len(plains[0]) + len(plains[1]) and r.plain() == plains[0] + plains[1]
    bad = bytearray(handmade(plains[2]))                                 # FHCRC: a candidate whose header the kernel refuses
    bad[12] ^= 0x20
    r = Run(mods, front + bytes(bad), sum(map(len, plains)))
    assert (r.status, r.error, r.nmembers, r.in_used) == (-3, "header crc mismatch", 2, len(front)), (r.status, r.error)
    r = Run(mods, front + members[2][:7], sum(map(len, plains)))         # 1f 8b and the file ends inside the header
    assert (r.status, r.nmembers, r.in_used) == (-5, 2, len(front) + 7), (r.status, r.in_used)


def test_first_member_that_is_not_gzip(mods, three):
    torch, inf, _, zr = mods
    plains, members = three
    for data in (zlib.compress(plains[0]) + members[1], b"\x1f\x8c" + members[0][2:], members[0][:2] + b"\x07" + members[0][3:],
                 b"\x1f", b"\x1f\x8b\x08", members[0][:len(members[0]) // 2], b""):
        src = place(torch, data, 5)
        ref = torch.full((len(plains[0]) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        want = inf.uncompress_large_dev(2, src, ref[1:1 + len(plains[0])])[:3]
        want_error = _error(zr)
        assert want[0] in (-3, -5)
        r = Run(mods, data, len(plains[0]), odd=5)
        assert (r.status, r.out_len, r.in_used, r.nmembers, r.rows) == want + (0, []), (data[:4], want)
        if want[0] == -3:
            assert r.error == want_error


def test_dst_cap_one_byte_short(mods, three):
    plains, members = three
    total = sum(map(len, plains))
    r = Run(mods, b"".join(members), total - 1)
    assert (r.status, r.nmembers) == (-5, 2) and r.out_len >= len(plains[0]) + len(plains[1]), (r.status, r.out_len)
    assert r.dst[:len(plains[0]) + len(plains[1])].cpu().numpy().tobytes() == plains[0] + plains[1]
    r = Run(mods, b"".join(members), len(plains[0]) - 1)                 # the first member does not fit
    assert (r.status, r.nmembers) == (-5, 0)
    r = Run(mods, bgzf_file(plains[0]), len(plains[0]) - 1)
    assert (r.status, r.nmembers) == (-5, -(-len(plains[0]) // BGZF_BLOCK) - 1), (r.status, r.nmembers)
    r = Run(mods, b"".join(members), total)                              # exactly enough
    assert (r.status, r.out_len) == (1, total)


def test_members_cap_below_the_count(mods, three):
    plains, members = three
    data = b"".join(members) + BGZF_EOF
    want = oracle_table(data)[0]
    for cap in (0, 1, 3, 4, 100):
        r = Run(mods, data, sum(map(len, plains)), members_cap=cap)
        assert (r.status, r.nmembers) == (1, 4) and r.rows == want[:cap], cap
        assert r.plain() == b"".join(plains)


# ---- single-member files, refusals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subblock", [False, True])
def test_a_single_member_is_the_single_call(mods, subblock):
    torch, inf, one, zr = mods
    big = _plain(24 * MiB + 4099, 50)                                    # synth's "sparse" class, the fourth segment, needs over 600 bytes
    cases = [("gzip-24MiB", gzip_file(big, "big.bin"), len(big)), ("handmade-100KiB", handmade(big[:100 * KiB]), 100 * KiB),
             ("own-compress2-8MiB", own_compress2(torch, one, 2, big[:8 * MiB]), 8 * MiB), ("empty", gzip_file(b"", ""), 0),
             ("cap-short", gzip_file(big[:MiB], ""), MiB - 1), ("flipped-isize", gzip_file(big[:MiB], "")[:-1] + b"\x77", MiB),
             ("cut", gzip_file(big[:MiB], "")[:-3], MiB)]
    for name, data, cap in cases:
        src = place(torch, data, 3)
        ref = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        want = inf.uncompress_large_dev(2, src, ref[9:9 + cap], subblock=subblock)[:3]
        want_error = _error(zr)
        r = Run(mods, data, cap, subblock=subblock)
        assert (r.status, r.out_len, r.in_used) == want, (name, want, r.status, r.out_len, r.in_used)
        assert r.nmembers == (1 if want[0] == 1 else 0), name
        if want[0] == 1:
            assert r.rows == oracle_table(data)[0] and torch.equal(r.dst[:r.out_len], ref[9:9 + r.out_len]), name
        if want[0] == -3:
            assert r.error == want_error, name


def test_refusals_launch_nothing(mods, three):
    torch, inf, _, zr = mods
    plains, members = three
    stream = torch.cuda.Stream()
    before = inf.workspace_bytes(stream)
    for flags in (2, 0x80000001, 0x10):
        r = Run(mods, b"".join(members), sum(map(len, plains)), flags=flags, stream=stream)
        assert (r.status, r.out_len, r.in_used, r.nmembers, r.rows) == (-3, 0, 0, 0, []) and r.untouched(), flags
        assert "flag" in r.error and inf.workspace_bytes(stream) == before
    lib = zr.rocm.lib()
    src = place(torch, members[0], 3)
    out_len, in_used, nm = C.c_uint64(5), C.c_size_t(6), C.c_size_t(7)
    for args in ((None, 10, src.data_ptr(), 10, None, 0), (src.data_ptr(), 10, None, 10, None, 0), (src.data_ptr(), 10, src.data_ptr(), 10, None, 1)):
        out_len.value, in_used.value, nm.value = 5, 6, 7
        rc = lib.zng_rocm_gunzip_members_dev(args[0], args[1], args[2], args[3], C.byref(out_len), C.byref(in_used), args[4], args[5],
                                             C.byref(nm), 0, C.c_void_p(stream.cuda_stream))
        assert (rc, out_len.value, in_used.value, nm.value) == (-3, 0, 0, 0), args
        assert inf.workspace_bytes(stream) == before
    assert struct.calcsize("<QQQQII") == C.sizeof(inf.GzipMember)


# ---- files made to hurt -------------------------------------------------------------------------------------------------------
def test_a_zero_free_run_of_fname_candidates(mods):
    """a candidate every four bytes of a stored member, each with FNAME set and no zero byte behind it: the header kernel is
    shown 4 KiB of each (gzip_members_plan.h kMembersHeaderLook), the member is decoded alone, the two behind it as planned"""
    hostile, plain = zero_free_stored_member(b"\x1f\x8b\x08\x08", 32)    # 1 MiB, about 260000 candidates
    two = [gzip_file(_plain(300 * KiB, 60), "second.txt"), handmade(_plain(50 * KiB, 61))]
    data = hostile + two[0] + two[1]
    r = Run(mods, data, len(plain) + 350 * KiB, odd=11)
    rows = _check_whole_file(r, data, "zero-free FNAME candidates")
    assert len(rows) == 3 and r.counters["candidates"] == len(scan(data)) > len(plain) // 4 - 100, r.counters
    assert r.counters["replans"] >= 1 and r.counters["small"] + r.counters["large"] == 3, r.counters


def test_a_header_longer_than_the_header_kernel_is_shown(mods, three):
    plains, members = three
    long_name = handmade(plains[2], name=b"n" * 5000)                    # a legal header of 5 KiB: cut for the finder, decoded alone
    data = members[0] + long_name + members[1] + long_name
    r = Run(mods, data, len(plains[0]) + len(plains[1]) + 2 * len(plains[2]), odd=13)
    rows = _check_whole_file(r, data, "long header")
    assert len(rows) == 4 and r.counters["replans"] == 0, r.counters


def test_more_candidates_than_are_tabled(mods):
    """more than 2^24 candidates (kMembersMaxCandidates): no table is built, the file goes through single calls member by member"""
    hostile, plain = zero_free_stored_member(b"\x1f\x8b\x08\x08", 2100)  # 65 MiB: a candidate every four bytes, 17.1 million
    assert len(plain) // 4 > (1 << 24) + 1000
    second = _plain(50 * KiB, 62)
    data = hostile + handmade(second) + BGZF_EOF
    r = Run(mods, data, len(plain) + len(second), odd=15)
    assert (r.status, r.out_len, r.in_used, r.nmembers) == (1, len(plain) + len(second), len(data), 3), (r.status, r.error)
    assert [row[:4] for row in r.rows] == [(0, len(hostile), 0, len(plain)), (len(hostile), len(data) - len(hostile) - 28, len(plain), len(second)),
                                           (len(data) - 28, 28, len(plain) + len(second), 0)]
    assert [row[4] for row in r.rows] == [zlib.crc32(plain), zlib.crc32(second), 0]
    assert r.plain() == plain + second
    assert r.counters == {"candidates": -1, "replans": 0, "small": 0, "large": 3}, r.counters
