"""zng_rocm_compress_members_header_dev and zng_rocm_compress_streams2_header_dev: device-resident gzip members with
deflateSetHeader's fields -- name, mtime, comment, FEXTRA, header CRC --, through the C ABI.  The batch is gzip_header_batch.py's:
every flag combination, header lengths around the frame kernel's workgroup (256) and around 4096, the 196621-byte maximum,
plaintexts of 0 bytes to several segments.

Oracles: the header is gzip_header_cases.model_header (struct and zlib.crc32); the deflate data is what
zng_rocm_compress_members_window_dev(2, ...) writes for the same jobs, level, strategy and window, byte for byte; the trailer is
zlib.crc32 and the length; CPython's zlib reads every member (wbits 31: it verifies FHCRC, CRC-32 and ISIZE)."""
import importlib
import zlib

import numpy as np
import pytest

import gzip_header_batch as gb
import gzip_header_cases as cases

pytestmark = pytest.mark.gpu
EINVAL, BUF_ERROR = -3, -5
COMBOS = [(0, 0, 15), (1, 0, 15), (6, 0, 15), (9, 0, 15), (6, 2, 15), (6, 0, 9)]      # (level, strategy, window_bits)


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.deflate"), importlib.import_module("zlib-ng_amd.inflate"), zr


@pytest.fixture(scope="module")
def batch(mods):
    return gb.batch(mods)


def test_the_batch_has_the_header_lengths_it_promises(batch):
    lens = [len(batch.model(i, 6, 0)) for i in range(batch.n)]
    assert tuple(lens[32:40]) == gb.EDGE_HEADS and lens[gb.BIG_AT] == 196621 and batch.n == 41
    assert sorted(batch.model(i, 6, 0)[3] for i in range(32)) == list(range(32))


@pytest.mark.parametrize("level,strategy,wbits", COMBOS)
def test_members_are_model_header_existing_deflate_data_trailer(mods, batch, level, strategy, wbits):
    f, plain_f = gb.written(mods, level, strategy, wbits)
    assert (f.status, plain_f.status) == (0, 0) and f.guard_ok and plain_f.guard_ok
    at = 0
    for i in range(batch.n):
        want = gb.want_member(batch, plain_f.member(i), i, level, strategy)
        assert f.off[i] == at, i                               # d_offsets: the running sums
        assert f.member(i) == want, (i, len(want))
        assert zlib.decompress(want, 31) == batch.plain[i]
        at += len(want)
    assert f.off[batch.n] == at == len(f.data)
    assert f.crc == [zlib.crc32(p) for p in batch.plain] == plain_f.crc


def test_file_goes_back_through_gunzip_members(mods, batch):
    torch, _, inf, _ = mods
    f, _ = gb.written(mods)
    total = sum(len(p) for p in batch.plain)
    src = torch.from_numpy(np.frombuffer(f.data, dtype=np.uint8).copy()).cuda()
    dst = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    st, out_len, in_used, rows, nmembers, _ = inf.gunzip_members_dev(src, dst[:total])
    assert (st, out_len, in_used, nmembers) == (1, total, len(f.data), batch.n)
    assert bytes(dst[:total].cpu().numpy()) == b"".join(batch.plain)
    assert [(r[0], r[1]) for r in rows] == [(f.off[i], f.off[i + 1] - f.off[i]) for i in range(batch.n)]


def test_null_heads_is_the_existing_call_byte_for_byte(mods, batch):
    torch, dfl, _, _ = mods
    _, plain_f = gb.written(mods)
    room = len(plain_f.data) + 100
    arena = torch.full((room,), 0xAB, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(batch.n + 1, dtype=torch.int64, device="cuda")
    checks = torch.zeros(batch.n, dtype=torch.int32, device="cuda")
    assert dfl.compress_members_dev(batch.jobs, batch.n, arena, offsets, 2, 6, 0, 0, checks) == 0
    torch.cuda.synchronize()
    n = int(offsets[-1])
    assert bytes(arena[:n].cpu().numpy()) == plain_f.data and [int(v) for v in offsets.cpu().tolist()] == plain_f.off
    assert [int(v) & 0xffffffff for v in checks.cpu().tolist()] == plain_f.crc
    assert plain_f.data[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3])


def test_three_and_more_rounds_give_the_file_of_one(mods, batch):
    f, _ = gb.written(mods)
    assert f.rounds == 1
    g = gb.File(mods, batch, 6, 0, 15, round_bytes=150000)
    assert g.status == 0 and g.rounds >= 3 and g.guard_ok
    assert g.data == f.data and g.off == f.off and g.crc == f.crc
    g = gb.File(mods, batch, 0, 0, 15, round_bytes=1)           # one job per round, stored
    assert g.status == 0 and g.rounds >= 3 and g.data == gb.written(mods, 0, 0, 15)[0].data


def test_dst_cap_inside_header_payload_and_trailer_writes_nothing_behind_it(mods, batch):
    f, _ = gb.written(mods)
    big = gb.BIG_AT
    caps = [f.off[5] + 3,                                        # inside a short header
            f.off[38] + 2000,                                    # inside a header of 4096 bytes
            f.off[big] + 100001,                                 # inside the longest header
            f.off[32] + 10 + 777,                                # inside a payload
            f.off[big + 1] - 5,                                  # inside the last trailer
            f.off[34] - 8,                                       # a trailer begins at the capacity
            0]
    for cap in caps:
        g = gb.File(mods, batch, 6, 0, 15, cap=cap)
        assert g.status == 0 and g.guard_ok, cap
        assert g.off == f.off and g.crc == f.crc                 # the scan goes on counting: the size the file needs
        assert g.room_bytes == f.data[:cap], cap


def streams2(mods, batch, level, strategy, wbits, shrink=None, heads=None):
    """the per-job-buffer form: every buffer exactly the bound, at an odd address inside 0xAB"""
    torch, dfl, _, zr = mods
    hd = batch.heads if heads is None else heads
    # (a refused header has 0 bytes: its buffer keeps the plain bound, so that the header is what the call refuses)
    caps = [dfl.compress_streams2_bound(len(p), 2) - 10 + max(dfl.gzip_header_bytes(hd[i]), 10) for i, p in enumerate(batch.plain)]
    offs, at = [], 0
    for k, cap in enumerate(caps):
        at += 16 + (gb.ODDS[(k + 3) % 8] - (at + 16)) % 16
        offs.append(at)
        at += cap
    arena = torch.full((at + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    results = torch.full((batch.n, 2), -0x54545455, dtype=torch.int32, device="cuda")
    jobs = dfl.stream_jobs(batch.views, [arena[o:o + c] for o, c in zip(offs, caps)])
    if shrink is not None:
        jobs[shrink].out_cap -= 1
    torch.cuda.synchronize()
    st = dfl.compress_streams2_header_dev(jobs, hd, batch.n, results, level, strategy, 0, None, wbits)
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    res = [(int(a) & 0xffffffff, int(b) & 0xffffffff) for a, b in results.cpu().tolist()]
    return st, host, offs, caps, res


def test_per_job_buffers_give_the_same_members(mods, batch):
    f, _ = gb.written(mods, 6, 0, 9)
    st, host, offs, caps, res = streams2(mods, batch, 6, 0, 9)
    assert st == 0
    mask = host == 0xAB
    for i in range(batch.n):
        want = f.member(i)
        assert res[i] == (len(want), zlib.crc32(batch.plain[i])) and len(want) <= caps[i]
        assert bytes(host[offs[i]:offs[i] + len(want)]) == want, i
        mask[offs[i]:offs[i] + len(want)] = True
    assert mask.all()                                            # nothing outside the members' own bytes


def test_out_cap_one_below_the_bound_is_refused_with_nothing_written(mods, batch):
    zr = mods[3]
    for shrink in (3, 37, gb.BIG_AT):
        st, host, _, _, res = streams2(mods, batch, 6, 0, 15, shrink=shrink)
        assert st == BUF_ERROR and (host == 0xAB).all() and res == [(0xABABABAB, 0xABABABAB)] * batch.n
        assert "zng_rocm_gzip_header_bytes" in zr.rocm.lib().zng_rocm_last_error().decode()


def test_refused_headers_leave_device_memory_and_results_untouched(mods, batch):
    torch, dfl, _, _ = mods

    def heads_with(i, change):
        hs = [cases.make_head(dfl, kw) for kw in batch.kws]
        change(hs[i])
        return dfl.gzip_headers(hs)

    def reserved(h):
        h.reserved = 7

    def extra_len(h):
        h.extra_len = 65536

    def dangling(h):
        h.extra, h.extra_len = None, 4

    def long_name(h):
        h.set_fields(None, b"n" * 65536, None)

    for i, change in ((0, reserved), (20, extra_len), (40, dangling), (33, long_name)):
        hs = heads_with(i, change)
        g = gb.File(mods, batch, 6, 0, 15, heads=hs)
        assert g.status == EINVAL and g.untouched, i
        st, host, _, _, res = streams2(mods, batch, 6, 0, 15, heads=hs)
        assert st == EINVAL and (host == 0xAB).all() and res == [(0xABABABAB, 0xABABABAB)] * batch.n, i
    for level, strategy, wbits in ((10, 0, 15), (6, 5, 15), (6, 0, 8), (6, 0, 16)):
        g = gb.File(mods, batch, level, strategy, wbits)
        assert g.status == EINVAL and g.untouched, (level, strategy, wbits)
