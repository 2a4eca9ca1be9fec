"""Crafted messages through every shape of the streaming checksum pass (checksum_kernel.h's stream_body), bit-exact against
CPython's zlib and, for constant fills, the closed form (tests/checksum_cases.py, which also holds the model of the pass and the
case families; tests/test_checksum_cases_cpu.py proves what they reach), with the project's oracle as a second reference on
every message of up to 128 KiB.

What stream_body does depends on how many 16 KiB units a workgroup owns.  zng_rocm_reserve_cus(CUs - G) runs the single-message
pass in G workgroups, so one workgroup pipelines, reduces its Adler sums mid-stream (on all-0xFF input too, and past the depth at
which an unreduced 32-bit sum would wrap) and weighs its CRC over 1024 and more units with a few MiB of input; the copy pass
(four units per register buffer) reaches its steady state the same way.  One test per family; each writes every case's two words
into its own row of one tensor and reads it back once.  reserve_cus is process-wide: every test restores 0, and so does the
module's fixture, which then checks one more call."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import checksum_cases as cc
from gpu_common import product, to_dev, torch_mod

pytestmark = pytest.mark.gpu
SENTINEL = 0xABABABAB
SENTINEL_I32 = SENTINEL - (1 << 32)
EINVAL = -3
GUARD = 64
ORACLE_MAX = 128 << 10


def _fused_probe(zr):
    """one small fused call against zlib"""
    torch = torch_mod()
    data = cc.pool()[:70001]
    out = torch.zeros(2, dtype=torch.int32, device="cuda")
    zr.adler32_crc32_dev(to_dev(data), out, adler=1, crc=0, length=70000, offset=1)
    return [v & 0xffffffff for v in out.tolist()] == [zlib.adler32(data[1:]), zlib.crc32(data[1:])]


@pytest.fixture(scope="module")
def zr():
    m = product()
    m.init()
    assert m.available()
    yield m
    m.reserve_cus(0)
    assert _fused_probe(m), "the checksum pass after reserve_cus went back to 0"


@pytest.fixture(scope="module")
def cus(zr):
    info = (4 * C.c_int32)()
    assert zr.rocm.lib().zng_rocm_device_info(info) == 0
    assert int(info[0]) == torch_mod().cuda.get_device_properties(0).multi_processor_count
    return int(info[0])


class Arenas:
    """device copies of what the fills read: the random pool, 0xFF and zeros (a hole or an impulse is set for one launch and taken
    back behind it, in stream order), all 16-byte aligned so that an offset's low four bits are the message's phase"""

    def __init__(self):
        torch = torch_mod()
        self.pool = to_dev(cc.pool())
        self.ff = torch.full((cc.DEEP_FF_UNITS * cc.UNIT + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        self.zero = torch.zeros((cc.IMPULSE_UNITS + 1) * cc.UNIT, dtype=torch.uint8, device="cuda")
        assert self.pool.data_ptr() % 16 == 0 and self.ff.data_ptr() % 16 == 0 and self.zero.data_ptr() % 16 == 0

    def launch(self, case, call):
        """call(buffer) with the case's bytes at buffer[phase : phase + n]"""
        kind, end = case.fill[0], case.phase + case.n
        if kind == "random":
            assert end <= self.pool.numel()
            call(self.pool)
        elif kind == "ramp":
            host = np.zeros(end, dtype=np.uint8)
            host[case.phase:] = cc.message(case)
            call(to_dev(host))
        else:
            buf, rest = (self.zero, 0) if kind == "impulse" else (self.ff, 0xFF)
            assert end <= buf.numel()
            if kind != "ff":
                at = case.phase + case.fill[1]
                buf[at] = case.fill[2] if kind == "impulse" else 0
            call(buf)
            if kind != "ff":
                buf[at] = rest


@pytest.fixture(scope="module")
def arenas(zr):
    return Arenas()


def _words(out):
    """rows of two words back from the device: the one synchronisation of a family (it surfaces any HIP error)"""
    return out.cpu().numpy().astype(np.int64) & 0xffffffff


def _want(case):
    a, c = cc.reference(case)
    return (a if case.which & 1 else SENTINEL, c if case.which & 2 else SENTINEL)      # the word not asked for stays untouched


def _check(cases, got, cus, oracle, extra=None):
    bad = []
    for i, c in enumerate(cases):
        if c.n <= ORACLE_MAX:                           # the project's oracle as a second reference where it costs nothing
            data = cc.message(c)
            ptr = data.ctypes.data if c.n else cc.pool().ctypes.data
            assert (oracle.oracle_adler32(c.adler_seed, ptr, c.n), oracle.oracle_crc32_braid(c.crc_seed, ptr, c.n)) == cc.reference(c), c.name
        row = (int(got[i, 0]), int(got[i, 1]))
        if row != _want(c) or (extra is not None and not extra[i]):
            bad.append((c.name, "got %08x %08x" % row, "want %08x %08x" % _want(c), "copy ok" if extra is None or extra[i] else "COPY WRONG",
                        cc.describe(cc.case_geometry(c, cus))))
    assert not bad, (len(bad), len(cases), bad[:6])


def _run_read(zr, arenas, cus, oracle, cases):
    """the read-only slots: which 1 -> adler32_dev, 2 -> crc32_dev (into the row's second word), 3 -> adler32_crc32_dev"""
    torch = torch_mod()
    out = torch.full((len(cases), 2), SENTINEL_I32, dtype=torch.int32, device="cuda")
    try:
        for i, c in enumerate(cases):
            assert not c.copy
            zr.reserve_cus(c.reserved)
            if c.which == 1:
                arenas.launch(c, lambda buf: zr.adler32_dev(buf, out[i], adler=c.adler_seed, length=c.n, offset=c.phase))
            elif c.which == 2:
                arenas.launch(c, lambda buf: zr.crc32_dev(buf, out[i, 1:], crc=c.crc_seed, length=c.n, offset=c.phase))
            else:
                arenas.launch(c, lambda buf: zr.adler32_crc32_dev(buf, out[i], adler=c.adler_seed, crc=c.crc_seed, length=c.n,
                                                                  offset=c.phase))
    finally:
        zr.reserve_cus(0)
    _check(cases, _words(out), cus, oracle)


def test_one_workgroup_read_only(zr, arenas, cus, oracle):
    """the whole pass in one workgroup: 1..481 units at two phases with and without tail bytes, all-0xFF through batches of 240 and
    through 1536 units (an unreduced batch of 1452 would wrap SR), 0xFF with one hole, the ramp"""
    _run_read(zr, arenas, cus, oracle, cc.one_workgroup_read_cases(cus))


def test_workgroup_count_sweep(zr, arenas, cus, oracle):
    """G = 1, 2, 3, 7, CUs - 4, CUs - 1, CUs workgroups around the unit counts where the split changes, a partial first unit, and
    the size at which the first of CUs - 4 workgroups needs the second digit of its end-of-body weight"""
    _run_read(zr, arenas, cus, oracle, cc.sweep_cases(cus))


def test_crc_impulses(zr, arenas, cus, oracle):
    """one 0x80 among zeros at the corners of lanes, units and the tail, in one and in three workgroups"""
    _run_read(zr, arenas, cus, oracle, cc.impulse_cases(cus))


def test_one_workgroup_copy(zr, arenas, cus, oracle):
    """fold_copy_dev in one workgroup: 0..6 and 59..120 pipelined groups of four units, 0..3 units behind them, batches of 240 and
    241; the destination holds the source and nothing around it changed"""
    torch = torch_mod()
    cases = cc.one_workgroup_copy_cases(cus)
    room = max(c.n for c in cases) + 2 * GUARD + 64
    dst = torch.empty(room, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    out = torch.full((len(cases), 2), SENTINEL_I32, dtype=torch.int32, device="cuda")
    copied = torch.zeros(len(cases), dtype=torch.bool, device="cuda")
    try:
        for i, c in enumerate(cases):
            assert c.copy and c.dst_shift % 16 == 0
            at = GUARD + c.dst_shift + c.phase
            dst[:at + c.n + GUARD] = 0xAA

            def call(buf, i=i, c=c, at=at):
                zr.fold_copy_dev(c.which, dst, buf, out[i], adler=c.adler_seed, crc=c.crc_seed, length=c.n, src_offset=c.phase,
                                 dst_offset=at)
                copied[i] = ((dst[at:at + c.n] == buf[c.phase:c.phase + c.n]).all() & (dst[at - GUARD:at] == 0xAA).all()
                             & (dst[at + c.n:at + c.n + GUARD] == 0xAA).all())
            zr.reserve_cus(c.reserved)
            arenas.launch(c, call)
    finally:
        zr.reserve_cus(0)
    got = _words(out)
    _check(cases, got, cus, oracle, copied.cpu().tolist())


def test_copy_edges(zr, arenas, cus, oracle):
    """every length 0..48 and around one unit at every phase, all three checks, every CU: each copy into its own slot of one arena
    of 0xAA, which must hold the source on [0, n) and 0xAA on the 64 bytes either side; and a copy between different phases is
    refused before anything is written"""
    torch = torch_mod()
    cases = cc.copy_edge_cases(cus)
    slots, at = [], 0
    for c in cases:
        slots.append(at)
        at += (2 * GUARD + c.phase + c.n + 15) // 16 * 16
    arena = torch.full((at,), 0xAA, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    out = torch.full((len(cases) + 1, 2), SENTINEL_I32, dtype=torch.int32, device="cuda")
    for i, c in enumerate(cases):
        assert c.reserved == 0 and c.fill == ("random",) and c.dst_shift == GUARD
        zr.fold_copy_dev(c.which, arena, arenas.pool, out[i], adler=c.adler_seed, crc=c.crc_seed, length=c.n, src_offset=c.phase,
                         dst_offset=slots[i] + GUARD + c.phase)
    # source at phase 3, destination at phase 4: ZNG_ROCM_EINVAL, the destination and the output words as they were
    refused = torch.full((1000 + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    rc = zr.rocm.lib().zng_rocm_fold_copy_dev(3, 1, 0, C.c_void_p(refused.data_ptr() + GUARD + 4), C.c_void_p(arenas.pool.data_ptr() + 3),
                                              1000, C.c_void_p(out[len(cases)].data_ptr()), zr.rocm._stream_ptr(None))
    assert rc == EINVAL, rc
    got = _words(out)
    assert (int(got[-1, 0]), int(got[-1, 1])) == (SENTINEL, SENTINEL) and bool((refused == 0xAA).all())
    host, src = arena.cpu().numpy(), cc.pool()
    copied = []
    for base, c in zip(slots, cases):
        d0 = base + GUARD + c.phase
        end = base + (2 * GUARD + c.phase + c.n + 15) // 16 * 16
        copied.append(bool((host[base:d0] == 0xAA).all() and (host[d0:d0 + c.n] == src[c.phase:c.phase + c.n]).all()
                           and (host[d0 + c.n:end] == 0xAA).all()) and end - (d0 + c.n) >= GUARD)
    _check(cases, got, cus, oracle, copied)


def test_many_messages_with_one_long_one(zr, arenas):
    """zng_rocm_checksums_dev: an empty message, 1 byte, 15 bytes, 1, 1024 and 1025 units, each at its own phase, beside 16 * 1024 + 1
    units of 0xFF that take G to its cap of 16 (so the short messages leave 15 or 16 workgroups without a unit); the same messages
    without the long one (G = 2) and the short ones alone (G = 1) give the same values"""
    torch = torch_mod()
    msgs = cc.many_messages()
    rand_bytes, total = cc.many_random_bytes()
    dev = torch.empty(total, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0
    dev[:rand_bytes] = arenas.pool[:rand_bytes]
    dev[rand_bytes:] = 0xFF                                             # the long message, built on the device
    runs = []
    for name, idx in cc.many_calls():
        G, geos = cc.many_geometry(idx)
        for which in (1, 2, 3):
            out = torch.full((len(idx), 2), SENTINEL_I32, dtype=torch.int32, device="cuda")
            zr.checksums_dev(which, dev, [msgs[i].offset for i in idx], [msgs[i].n for i in idx], out,
                             [msgs[i].adler_seed for i in idx], [msgs[i].crc_seed for i in idx])
            runs.append((name, idx, which, G, geos, out))
    got = _words(torch.cat([r[-1] for r in runs]))
    want = [cc.many_reference(m) for m in msgs]
    first, row, bad = {}, 0, []
    for name, idx, which, G, geos, _ in runs:
        for i, geo in zip(idx, geos):
            have = (int(got[row, 0]), int(got[row, 1]))
            row += 1
            expect = (want[i][0] if which & 1 else SENTINEL, want[i][1] if which & 2 else SENTINEL)
            if have != expect or first.setdefault((i, which), have) != have:
                bad.append((name, msgs[i].name, "which %d" % which, "got %08x %08x" % have, "want %08x %08x" % expect, cc.describe(geo)))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("fmt", [1, 2])
def test_device_built_descriptor_of_maximal_bytes(zr, fmt):
    """fill_check_descriptor gives a message one workgroup whatever its length: 8 MiB of 0xFF (512 units, two mid-stream
    reductions) through the many-stream compress entry point as a stored zlib / gzip stream, whose trailer and result word must
    carry zlib's check value and which CPython must accept"""
    torch = torch_mod()
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    n = cc.DESCRIPTOR_BYTES
    (w,) = cc.geometry(n, 3, 1, cc.ROWS).wgs
    assert w.folds == 2 and w.deepest == cc.BATCH_MAX
    src = torch.full((n + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    cap = dfl.compress_streams2_bound(n, fmt)
    dst = torch.full((cap + 2 * GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    results = torch.full((1, 2), SENTINEL_I32, dtype=torch.int32, device="cuda")
    jobs = dfl.stream_jobs([src[3:3 + n]], [dst[GUARD + 5:GUARD + 5 + cap]])
    status = dfl.compress_streams2_dev(jobs, 1, results, fmt, level=0)
    assert status == 0, (status, zr.rocm.lib().zng_rocm_last_error().decode())
    nbytes, check = (int(v) & 0xffffffff for v in results.cpu().tolist()[0])
    assert nbytes <= cap
    host = dst.cpu().numpy()
    member = host[GUARD + 5:GUARD + 5 + nbytes].tobytes()
    assert (host[:GUARD + 5] == 0xAB).all() and (host[GUARD + 5 + nbytes:] == 0xAB).all()
    plain = b"\xff" * n
    if fmt == 1:
        want = zlib.adler32(plain)
        assert want == cc.adler_constant(0xFF, n, 1)
        assert int.from_bytes(member[-4:], "big") == want, cc.describe(cc.geometry(n, 3, 1, cc.ROWS))
    else:
        want = zlib.crc32(plain)
        assert int.from_bytes(member[-8:-4], "little") == want, cc.describe(cc.geometry(n, 3, 1, cc.ROWS))
        assert int.from_bytes(member[-4:], "little") == n
    assert check == want
    assert zlib.decompress(member, 15 if fmt == 1 else 31) == plain
