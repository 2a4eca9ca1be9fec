"""The batch the GPU tests of the gzip header calls share (test_gpu_gzip_header_write.py, test_gpu_gzip_header_read.py): about
40 jobs of text from data_lcet10.txt with a header each, the file zng_rocm_compress_members_header_dev writes for them, and the
file the same call without headers writes -- each made once per (level, strategy, window) and kept.

  jobs 0..31    every combination of the five flag bits, empty and small fields, plaintexts of 0, 1 and 300 bytes
  jobs 32..39   headers of 10, 11, 255, 256, 257, 4095, 4096, 4097 bytes (256: the frame kernel's workgroup; 4096: the step of
                the zero search), plaintexts around the block cut of 61440 and one of 200000 bytes
  job 40        the 196621-byte maximum in front of 205000 bytes
Every plaintext sits at an odd device address."""
import os
import struct
import zlib

import numpy as np

import gzip_header_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SIZES = (0, 1, 300)
EDGE_HEADS = (10, 11, 255, 256, 257, 4095, 4096, 4097)
EDGE_SIZES = (61439, 61440, 61441, 300, 1, 0, 300, 200000)
BIG_AT = 32 + len(EDGE_HEADS)
ODDS = (5, 1, 15, 8, 3, 0, 11, 6)
_cache = {}


def head_fields():
    kws = [cases.fields(flg, size=flg % 2, seed=flg) for flg in range(32)]
    for total in EDGE_HEADS:
        kws.append(cases.fields(0, 0, total) if total == 10 else cases.padded(total, 8, total) if total == 11 else
                   cases.padded(total, (8 | 16 | 2, 8 | 2, 16)[total % 3], total))
    kws.append(cases.biggest(41))
    return kws


class Batch:
    def __init__(self, torch, dfl):
        with open(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "data_lcet10.txt"), "rb") as f:
            lcet = f.read()
        self.kws = head_fields()
        sizes = [SMALL_SIZES[i % 3] for i in range(32)] + list(EDGE_SIZES) + [205000]
        self.n = len(sizes)
        assert self.n == len(self.kws) == BIG_AT + 1
        self.plain, self.off = [], []
        arena = bytearray()
        for i, n in enumerate(sizes):
            start = (i * 29989) % (len(lcet) - n)
            gap = 16 + (ODDS[i % 8] - (len(arena) + 16)) % 16
            arena += b"\xab" * gap
            self.off.append(len(arena))
            self.plain.append(lcet[start:start + n])
            arena += self.plain[-1]
        arena += b"\xab" * 64
        self.src = torch.from_numpy(np.frombuffer(bytes(arena), dtype=np.uint8).copy()).cuda()
        self.views = [self.src[o:o + len(p)] for o, p in zip(self.off, self.plain)]
        self.heads = dfl.gzip_headers([cases.make_head(dfl, kw) for kw in self.kws])
        self.jobs = dfl.stream_jobs(self.views)

    def model(self, i, level, strategy):
        return cases.model_header(level, strategy, **self.kws[i])


def batch(mods):
    if "batch" not in _cache:
        _cache["batch"] = Batch(mods[0], mods[1])
    return _cache["batch"]


class File:
    """one zng_rocm_compress_members_header_dev call over the batch into an arena of 0xAB of `cap` bytes (None: room for all) at
    an odd address; .data = the bytes of the file that fit, .guard_ok = no byte at or behind the capacity changed"""

    def __init__(self, mods, b, level, strategy, wbits, with_heads=True, round_bytes=0, cap=None, heads=None):
        torch, dfl = mods[0], mods[1]
        room = sum(dfl.compress_streams2_bound(len(p), 2) + 196621 for p in b.plain) if cap is None else cap
        self.arena = torch.full((room + 3 + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
        dst = self.arena[3:3 + room]
        self.offsets = torch.full((b.n + 1,), -1, dtype=torch.int64, device="cuda")
        self.checks = torch.full((b.n,), -0x54545455, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        hd = (b.heads if heads is None else heads) if with_heads else None
        self.status = dfl.compress_members_header_dev(b.jobs, hd, b.n, dst, self.offsets, level, strategy, round_bytes, self.checks,
                                                      None, wbits)
        self.rounds = dfl.compress_streams2_last_rounds()
        torch.cuda.synchronize()
        host = self.arena.cpu().numpy()
        self.off = [int(v) for v in self.offsets.cpu().tolist()]
        self.crc = [int(v) & 0xffffffff for v in self.checks.cpu().tolist()]
        self.guard_ok = bool((host[:3] == 0xAB).all()) and bool((host[3 + room:] == 0xAB).all())
        self.untouched = bool((host == 0xAB).all()) and self.off == [-1] * (b.n + 1) and self.crc == [0xABABABAB] * b.n
        self.data = bytes(host[3:3 + min(room, max(self.off[-1], 0))]) if self.status == 0 else b""
        self.room_bytes = bytes(host[3:3 + room])
        self.dev = dst

    def member(self, i):
        return self.data[self.off[i]:self.off[i + 1]]


def written(mods, level=6, strategy=0, wbits=15):
    """(the file with headers, the file of the call without) for one combination, made once"""
    key = (level, strategy, wbits)
    if key not in _cache:
        b = batch(mods)
        _cache[key] = (File(mods, b, level, strategy, wbits), File(mods, b, level, strategy, wbits, with_heads=False))
    return _cache[key]


def want_member(b, plain_member, i, level, strategy):
    """model header + the deflate data of the member the call without headers wrote + CRC-32 and ISIZE"""
    p = b.plain[i]
    return b.model(i, level, strategy) + plain_member[10:-8] + struct.pack("<II", zlib.crc32(p), len(p))
