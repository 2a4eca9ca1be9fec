"""What the zlib / gzip framing costs on top of the large device inflaters: the framed calls
zng_rocm_uncompress_large_streams_dev / zng_rocm_uncompress_large_dev against the raw calls on the payloads alone, and the
check pass on its own (zng_rocm_checksums_cut_dev) against a single-message pass over one buffer of the same total size.

Everything device-resident and warm; the ways of a leg alternate inside one process, one untimed warm-up call each, then
--reps (5) timings each; a figure is the best timing, its spread max - min.

  batch         the mixed gzip batch of tests/wrapped_members.py (the one tests/test_gpu_uncompress_large.py checks): raw batch, framed batch, check_pass
                (sub-messages + fold over the same outputs), check_floor (zng_rocm_crc32_dev over ONE buffer of the batch's
                total output size).  The one timing condition: check_pass_ms <= 2 x check_floor_ms.
  one_stream    --mib (256) MiB of synth.silesia_like, this library's level 6, as a gzip member through
                zng_rocm_uncompress_large_dev against zng_rocm_inflate_large_pieces_dev on its payload
  long_header   a gzip member with an 8 MiB FNAME and FHCRC in front of a 4 MiB payload (test 4): the framed batch call on
                it alone; the header kernels themselves are read off a rocprofv3 --kernel-trace --stats run of
                `--only long_header`

    python tools/uncompress_large_rate.py [--mib 256] [--reps 5] [--only batch|one_stream|long_header] [--out FILE.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncompress_large_rate_v1.json"))
    a = ap.parse_args()
    import torch
    import synth
    import wrapped_members as fixture
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    inf = importlib.import_module("zlib-ng_amd.inflate")
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    one = importlib.import_module("zlib-ng_amd.oneshot")
    rocm = zr.rocm
    lib = rocm.lib()
    st = torch.cuda.Stream()
    sp = C.c_void_p(st.cuda_stream)

    def timings(ways):
        per = {k: [] for k in ways}
        for fn in ways.values():                          # warm-up: allocates the scratch
            fn()
        st.synchronize()
        for _ in range(a.reps):
            for k, fn in ways.items():
                st.synchronize()
                t0 = time.perf_counter()
                fn()
                st.synchronize()
                per[k].append(time.perf_counter() - t0)
        return {k: dict(ms=round(min(v) * 1e3, 4), spread_ms=round((max(v) - min(v)) * 1e3, 4), timings_ms=[round(x * 1e3, 4) for x in v])
                for k, v in per.items()}

    out = {"tool": "tools/uncompress_large_rate.py", "device": torch.cuda.get_device_name(0), "reps": a.reps}

    def batch_leg(members, fmt):
        hl = [inf.wrapper_parse(fmt, m.data)[1] for m in members]
        bufs = [m.dst(torch) for m in members]
        n = len(members)
        framed = inf.large_jobs([m.src for m in members], [b[1] for b in bufs])
        raw = inf.large_jobs([m.src[h:] for m, h in zip(members, hl)], [b[1] for b in bufs])
        fp, rp = C.cast(framed, C.c_void_p), C.cast(raw, C.c_void_p)
        total = sum(len(m.plain) for m in members)
        check_jobs = (rocm.CheckJob * n)()
        for i, (m, b) in enumerate(zip(members, bufs)):
            check_jobs[i].buf, check_jobs[i].len, check_jobs[i].adler, check_jobs[i].crc = b[1].data_ptr(), len(m.plain), 1, 0
        checks = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        flat = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        which = 1 if fmt == 1 else 2

        def raw_batch():
            assert lib.zng_rocm_inflate_large_streams_dev(rp, n, 0, 0, sp) == 0

        def framed_batch():
            assert lib.zng_rocm_uncompress_large_streams_dev(fmt, fp, n, 0, 0, sp) == 0

        def check_pass():
            assert lib.zng_rocm_checksums_cut_dev(which, C.byref(check_jobs), n, rocm._dev_ptr(checks), sp) == 0

        def check_floor():
            fn = lib.zng_rocm_adler32_dev if fmt == 1 else lib.zng_rocm_crc32_dev
            assert fn(1 if fmt == 1 else 0, rocm._dev_ptr(flat), total, rocm._dev_ptr(checks), sp) == 0

        with torch.cuda.stream(st):
            row = timings({"raw_batch": raw_batch, "framed_batch": framed_batch, "check_pass": check_pass, "check_floor": check_floor})
            framed_batch()
            st.synchronize()
        assert all(j.status == 1 and j.out_len == len(m.plain) and j.in_used == m.first for j, m in zip(framed[:n], members))
        assert all(j.status == 1 for j in raw[:n])
        row.update(jobs=n, output_bytes=total, jobs_on_device=sum(1 for j in framed[:n] if j.parts > 0),
                   rounds=int(lib.zng_rocm_inflate_large_last_rounds()),
                   framed_minus_raw_ms=round(row["framed_batch"]["ms"] - row["raw_batch"]["ms"], 4),
                   check_pass_ms=row["check_pass"]["ms"], check_floor_ms=row["check_floor"]["ms"])
        row["fixed_part_ms"] = round(row["framed_minus_raw_ms"] - row["check_pass_ms"], 4)
        return row

    if a.only in (None, "batch"):
        members = fixture.mixed(torch, dfl, one, 2)
        row = batch_leg(members, 2)
        row["check_pass_within_2x_floor"] = bool(row["check_pass_ms"] <= 2 * row["check_floor_ms"])
        out["batch"] = row
        print("batch", json.dumps(row), flush=True)
        print("check_pass_ms %.4f <= 2 x check_floor_ms %.4f: %s" % (row["check_pass_ms"], row["check_floor_ms"],
                                                                    row["check_pass_within_2x_floor"]), flush=True)
        del members

    if a.only in (None, "one_stream"):
        total = a.mib * MiB
        plain = synth.silesia_like(total, seed=2026)
        want = torch.from_numpy(plain).cuda()
        comp, n = dfl.deflate_dev(want, level=6)
        head = bytes([0x1f, 0x8b, 8, 8, 0, 0, 0, 0, 0, 3]) + b"cfg3.bin\0"
        member = torch.zeros(len(head) + n + 8 + 64, dtype=torch.uint8, device="cuda")
        member[:len(head)] = torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()).cuda()
        member[len(head):len(head) + n] = comp[:n]
        crc = torch.zeros(2, dtype=torch.int32, device="cuda")
        zr.crc32_dev(want, crc)
        torch.cuda.synchronize()
        trailer = struct.pack("<II", int(crc[0]) & 0xffffffff, total & 0xffffffff)
        member[len(head) + n:len(head) + n + 8] = torch.from_numpy(np.frombuffer(trailer, dtype=np.uint8).copy()).cuda()
        mlen = len(head) + n + 8
        dst = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        out_len, in_used = C.c_uint64(0), C.c_size_t(0)
        torch.cuda.synchronize()

        def raw_pieces():
            assert lib.zng_rocm_inflate_large_pieces_dev(C.c_void_p(member.data_ptr() + len(head)), n + 8, None, 0, rocm._dev_ptr(dst),
                                                         total, C.byref(out_len), C.byref(in_used), 0, 0, sp) == 1

        def framed():
            assert lib.zng_rocm_uncompress_large_dev(2, rocm._dev_ptr(member), mlen, None, 0, rocm._dev_ptr(dst), total,
                                                     C.byref(out_len), C.byref(in_used), 0, 0, sp) == 1

        def check_whole():
            assert lib.zng_rocm_crc32_dev(0, rocm._dev_ptr(dst), total, rocm._dev_ptr(crc), sp) == 0

        with torch.cuda.stream(st):
            row = timings({"raw_pieces": raw_pieces, "framed": framed, "check_whole": check_whole})
            dst.zero_()
            framed()
            st.synchronize()
            assert (out_len.value, in_used.value) == (total, mlen) and torch.equal(dst[:total], want)
        row.update(output_bytes=total, compressed_bytes=n, parts=int(lib.zng_rocm_inflate_large_last_parts()),
                   framed_minus_raw_ms=round(row["framed"]["ms"] - row["raw_pieces"]["ms"], 4))
        out["one_stream"] = row
        print("one_stream", json.dumps(row), flush=True)
        del want, dst, member, comp

    if a.only in (None, "long_header"):
        p = synth.silesia_like(4 * MiB, seed=0x501).tobytes()
        name = np.random.default_rng(0x501).integers(1, 256, size=8 * MiB, dtype=np.uint8).tobytes()
        head = bytes([0x1f, 0x8b, 8, 8 | 2, 0, 0, 0, 0, 0, 3]) + name + b"\0"
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
        m = fixture.Member(torch, "8MiB-name", head + fixture.raw(p) + fixture.trailer(2, p), p, 3)
        short = fixture.Member(torch, "no-name", fixture.wrap(2, p), p, 3)
        rows = {}
        for label, mem in (("long_header", m), ("same_payload_plain_header", short)):
            whole, dst = mem.dst(torch)
            jobs = inf.large_jobs([mem.src], [dst])
            jp = C.cast(jobs, C.c_void_p)

            def call():
                assert lib.zng_rocm_uncompress_large_streams_dev(2, jp, 1, 0, 0, sp) == 0

            with torch.cuda.stream(st):
                rows[label] = timings({"framed": call})["framed"]
            assert jobs[0].status == 1 and jobs[0].in_used == len(mem.data)
        out["long_header"] = dict(header_bytes=len(head), **rows,
                                  long_minus_plain_ms=round(rows["long_header"]["ms"] - rows["same_payload_plain_header"]["ms"], 4))
        print("long_header", json.dumps(out["long_header"]), flush=True)

    lib.zng_rocm_stream_release(sp)
    if a.out and not a.only:                             # a single leg (a profiler run) leaves the report alone
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
