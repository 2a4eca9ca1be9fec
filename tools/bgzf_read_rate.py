"""What BGZF random access costs beside the whole-file decode it replaces.

One file, device-resident: BGZF, --mib (1024) MiB of plaintext from synth.silesia_like in blocks of 65280 bytes compressed by
CPython's zlib at level 6, and the 28-byte end-of-file block (a stretch of distinct members is compressed on the host and
repeated on the device up to the size: members are independent, so the file is valid and no two neighbours are alike).

Four ways over it, alternating inside one process, one untimed warm-up each, then --reps (5) timings each over rotating
buffers (--rotate 2 copies of the file and of every destination, so that no call finds its bytes in the Infinity Cache from
the call before); a figure is the MEDIAN host time around a call that ends in a synchronise, with min and max beside it:

  whole     zng_rocm_gunzip_members_dev on the whole file: before this tool's calls existed, the only way to get the rows, and
            the only way to serve any range (decode everything, slice)
  index     zng_rocm_bgzf_index_dev on the same file
  read_4k   zng_rocm_bgzf_read_dev: --ranges (4096) ranges of 4 KiB at random offsets (seeded), one call
  read_1m   the same with ranges of 1 MiB

Recorded, not gated: index / whole and read_4k / whole (expected well below 1), read_1m / whole, the read calls' counters and
bytes delivered.  Every read is checked: all statuses 1, and the first, the last and 30 other ranges byte for byte against
the plaintext; the index's rows are the rows the whole-file call reports.

    python tools/bgzf_read_rate.py [--mib 1024] [--reps 5] [--ranges 4096] [--out FILE.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=2)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_read_rate_v1.json"))
    a = ap.parse_args()
    assert a.reps >= 1 and a.rotate >= 1 and a.ranges >= 32 and a.mib >= 2
    import torch
    import synth
    import gzip_files
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    inf = importlib.import_module("zlib-ng_amd.inflate")
    rocm = zr.rocm
    lib = rocm.lib()
    st = torch.cuda.Stream()
    sp = C.c_void_p(st.cuda_stream)
    block = gzip_files.BGZF_BLOCK

    unit_mib = min(64, a.mib)
    p = synth.silesia_like(unit_mib * MiB // block * block, seed=0xB6F)
    raw = p.tobytes()
    stretch = [gzip_files.bgzf_block(raw[at:at + block]) for at in range(0, len(raw), block)]
    unit = b"".join(stretch)
    repeat = max(1, a.mib // unit_mib)
    total, plain_len = len(unit) * repeat + len(gzip_files.BGZF_EOF), len(raw) * repeat
    nm = len(stretch) * repeat + 1
    unit_dev = torch.from_numpy(np.frombuffer(unit, dtype=np.uint8).copy()).cuda()
    plain_dev = torch.from_numpy(p).cuda()
    srcs, wholes = [], []
    for _ in range(a.rotate):
        s = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        for r in range(repeat):
            s[r * len(unit):(r + 1) * len(unit)] = unit_dev
        s[len(unit) * repeat:total] = torch.from_numpy(np.frombuffer(gzip_files.BGZF_EOF, dtype=np.uint8).copy()).cuda()
        srcs.append(s)
        wholes.append(torch.zeros(plain_len + 64, dtype=torch.uint8, device="cuda"))

    whole_rows, index_rows = (inf.GzipMember * nm)(), (inf.GzipMember * nm)()
    out_len, in_used, nmembers, plain_out = C.c_uint64(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)

    def whole(k):
        assert lib.zng_rocm_gunzip_members_dev(rocm._dev_ptr(srcs[k % a.rotate]), total, rocm._dev_ptr(wholes[k % a.rotate]), plain_len,
                                               C.byref(out_len), C.byref(in_used), C.cast(whole_rows, C.c_void_p), nm, C.byref(nmembers), 0,
                                               sp) == 1

    def index(k):
        assert lib.zng_rocm_bgzf_index_dev(rocm._dev_ptr(srcs[k % a.rotate]), total, C.cast(index_rows, C.c_void_p), nm, C.byref(nmembers),
                                           C.byref(plain_out), C.byref(in_used), sp) == 0

    rng = np.random.default_rng(0xB6F2)
    legs = {}
    for name, length in (("read_4k", 4096), ("read_1m", MiB)):
        uoffs = [int(u) for u in rng.integers(0, plain_len - length, size=a.ranges)]
        dsts = [torch.zeros(a.ranges * length + 64, dtype=torch.uint8, device="cuda") for _ in range(a.rotate)]
        tables = []
        for d in dsts:
            rs = (inf.BgzfRange * a.ranges)()
            for i, u in enumerate(uoffs):
                rs[i] = inf.BgzfRange(u, length, d.data_ptr() + i * length, 0, 0, None)
            tables.append(rs)
        legs[name] = (length, uoffs, dsts, tables)

    def reader(name):
        length, uoffs, dsts, tables = legs[name]

        def run(k):
            assert lib.zng_rocm_bgzf_read_dev(rocm._dev_ptr(srcs[k % a.rotate]), total, C.cast(index_rows, C.c_void_p), nm,
                                              C.cast(tables[k % a.rotate], C.c_void_p), a.ranges, 0, sp) == 0
        return run

    ways = {"whole": whole, "index": index, "read_4k": reader("read_4k"), "read_1m": reader("read_1m")}
    per = {k: [] for k in ways}
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for fn in ways.values():                          # warm-up: allocates the scratch (index before the readers: their rows)
            fn(0)
        st.synchronize()
        for rep in range(a.reps):
            for k, fn in ways.items():
                st.synchronize()
                t0 = time.perf_counter()
                fn(rep + 1)
                st.synchronize()
                per[k].append(time.perf_counter() - t0)
        # what was computed
        assert (nmembers.value, plain_out.value, in_used.value) == (nm, plain_len, total)
        same = lambda x, y: (x.src_off, x.src_len, x.dst_off, x.out_len, x.crc, x.bgzf) == (y.src_off, y.src_len, y.dst_off, y.out_len,  # noqa: E731
                                                                                          y.crc, y.bgzf)
        assert all(same(x, y) for x, y in zip(whole_rows, index_rows))
        counters = {}
        for name in ("read_4k", "read_1m"):
            length, uoffs, dsts, tables = legs[name]
            for d in dsts:
                d.zero_()
            ways[name](0)
            st.synchronize()
            counters[name] = {k: int(getattr(lib, "zng_rocm_bgzf_read_last_" + k)()) for k in ("decoded", "direct", "rounds")}
            assert all(r.status == 1 and r.out_len == length and r.msg is None for r in tables[0])
            for i in [0, a.ranges - 1] + [int(v) for v in rng.integers(0, a.ranges, size=30)]:
                u, got = uoffs[i], dsts[0][i * length:(i + 1) * length]
                lo = u % len(raw)                         # the plaintext repeats every len(raw) bytes
                want = torch.cat([plain_dev[lo:], plain_dev])[:length] if lo + length > len(raw) else plain_dev[lo:lo + length]
                assert torch.equal(got, want), (name, i, u)

    def figure(v, nbytes):
        med = statistics.median(v)
        return dict(ms=round(med * 1e3, 4), min_ms=round(min(v) * 1e3, 4), max_ms=round(max(v) * 1e3, 4), gbps=round(nbytes / med / 1e9, 3))

    out = {"tool": "tools/bgzf_read_rate.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rotate": a.rotate,
           "figure": "median of reps, host clock around a call that ends in a synchronise; GB/s of bytes delivered",
           "members": nm, "file_bytes": total, "plain_bytes": plain_len, "ranges": a.ranges,
           "whole": figure(per["whole"], plain_len), "index": figure(per["index"], total)}
    for name in ("read_4k", "read_1m"):
        out[name] = figure(per[name], a.ranges * legs[name][0])
        out[name].update(range_bytes=legs[name][0], delivered_bytes=a.ranges * legs[name][0], counters=counters[name])
    w = out["whole"]["ms"]
    out["index_over_whole"] = round(out["index"]["ms"] / w, 4)
    out["read_4k_over_whole"] = round(out["read_4k"]["ms"] / w, 4)
    out["read_1m_over_whole"] = round(out["read_1m"]["ms"] / w, 4)
    lib.zng_rocm_stream_release(sp)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
