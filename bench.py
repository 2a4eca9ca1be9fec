#!/usr/bin/env python3
"""bench.py -- headline measurement of the arch/rocm hot path on MI355X.

Top-level line (BASELINE.json configs[1]): crc32 + adler32 over a 1 GiB synthetic buffer that is already resident
in HBM, block-parallel with on-device combine.  One "step" = one fused pass of `zng_rocm_adler32_crc32_dev` over
the rank's 1 GiB shard (both checksums, bytes read once).  N > 1: weak scaling -- every rank owns its own 1 GiB
shard of one N GiB logical buffer; the only exchange is the all-gather of {adler, crc, len} (16 bytes per rank over
RCCL) followed by the ordered on-device combine.

With --full the same line carries a `streams` object at every N (BASELINE.json configs[4], the north_star's multi-stream
curve): 4096 independent 1 MiB streams, level-1 class, sharded over the N ranks (strong scaling), the {clen,
adler32, ulen} table all-gathered over RCCL; `streams.value` at N = 1, 2, 4, 8 is the 1 -> 8 GPU scaling curve.
And the two single-stream members of the metric, `deflate_lvl6` (configs[3]) and `inflate` (configs[2]): one 256 MiB
stream per GPU (a single stream does not shard: replicas at N > 1).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   (N > 1, the driver's form)
`python bench.py --gpus N` with N > 1 and no launcher around it starts its own N ranks (self_launch(): a child
`torch.distributed.run`, started before this process has imported torch or touched HIP) and relays rank 0's line.
Rank 0 prints ONE JSON line.

A plain run does only what the top-level line needs: set-up, the untimed settle launches, W warm-up steps, K timed
steps, the line.  `--full` adds everything else: the single-checksum kernel rates, the device-copy ceiling, the CPU
baseline and its check against the GPU result, and the `streams` / `deflate_lvl6` / `inflate` objects.
`--dump-outputs DIR` writes what the timed path returned in its last step as DIR/<name>.npy (float64): `checksums`
= {adler32, crc32} of rank 0's shard, and at N > 1 (or ZNG_BENCH_FORCE_DIST=1) `combined` = the ordered combine over
all ranks; `--workload streams` writes `streams_table`, the {clen, adler32, ulen} row of every stream.  The inputs are
seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

METRIC = "GB/s input throughput (adler32, crc32, deflate lvl6, inflate) @1/2/4/8 GPU vs CPU ref"
HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
SHARD_BYTES = 1 << 30           # cfg2: 1 GiB per GPU
SEED = 0x5EED0002
# The kernel reaches its steady clock only after a while: a few hundred launches on an idle box (tools/micro/fused_steady.py:
# 5.39 -> 6.10 TB/s over the first ~100), but about TWO SECONDS when the process starts within a few seconds of a heavy GPU
# job, as it does behind the test suite -- there the same kernel read 0.79 of peak behind 300 or 1000 settle launches, 0.806
# / 0.816 behind 2300 / 3500, 0.825-0.834 behind 12000, and 0.828 behind 600 after a 12 s pause (round 3, five boxes).  The
# settle phase below is UNTIMED and disclosed in the line (`settle_launches`): it runs before the W warm-up steps, so the K
# timed steps measure the steady state whatever ran before.
SETTLE_LAUNCHES = 12000
TRACE_STRIDE = 8                # every 8th launch of the timed loop carries dispatch-attached HIP events (its own start / stop)

# the REAL reference (zlib-ng 2.2.2, cmake build, runtime dispatch to AVX-512 VNNI /
# VPCLMULQDQ), measured in the survey container on one thread -- quoted for context, not measured by this script
REFERENCE_CONTAINER = {
    "what": "zlib-ng 2.2.2 itself, 1 thread, Xeon @2.1 GHz, survey container (BASELINE.md section 2); not re-measured here",
    "adler32_GBps": 7.5, "crc32_GBps": 9.8, "deflate_level1_GBps": 0.171, "deflate_level6_GBps": 0.044,
    "inflate_out_GBps": [0.318, 0.516],
}


def host_threads():
    """host cores this process may really use: its CPU affinity, capped by the control group's CPU quota"""
    try:
        n = max(1, len(os.sched_getaffinity(0)))
    except AttributeError:
        n = max(1, os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def system_zlib_probe(ptr, n, reps):
    """when the box has a system libz-ng.so.2 / libz.so.1, time ITS adler32 / crc32 on the same bytes
    (one thread), labelled by zlibVersion() -- whatever it is, it is not this repository's code.  None when neither loads."""
    import ctypes as C
    for name, pre in (("libz-ng.so.2", "zng_"), ("libz.so.1", "")):
        try:
            lib = C.CDLL(name)
            ver = getattr(lib, ("zlibng_version" if pre else "zlibVersion"))
            ver.restype = C.c_char_p
            ad, cr = getattr(lib, pre + "adler32_z", None) or getattr(lib, pre + "adler32"), \
                getattr(lib, pre + "crc32_z", None) or getattr(lib, pre + "crc32")
        except (OSError, AttributeError):
            continue
        for f in (ad, cr):
            f.restype = C.c_ulong
            f.argtypes = [C.c_ulong, C.c_void_p, C.c_size_t]
        chunk = 1 << 30 if ad.__name__.endswith("_z") else (1 << 31) - 1
        ta, tc = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            a, off = 1, 0
            while off < n:
                ln = min(chunk, n - off)
                a = ad(a, ptr + off, ln)
                off += ln
            t1 = time.perf_counter()
            c, off = 0, 0
            while off < n:
                ln = min(chunk, n - off)
                c = cr(c, ptr + off, ln)
                off += ln
            t2 = time.perf_counter()
            ta.append(t1 - t0)
            tc.append(t2 - t1)
        return {"library": name, "version": (ver() or b"?").decode(), "cores": 1, "adler32_GBps": round(n / 1e9 / statistics.median(ta), 3),
                "crc32_GBps": round(n / 1e9 / statistics.median(tc), 3), "checks": [a & 0xffffffff, c & 0xffffffff]}
    return None


def cpu_baseline(host_view, zr, reps=5):
    """The CPU checker timed on this box's host cores over the step's own bytes: adler32 = the oracle port of
    adler32_c.c, crc32 = the reference's crc32_braid_c.c (oracle/_ref) when it was built.  Two figures (BASELINE.md
    section 3): one thread, and T threads each on its own contiguous slice folded with the combine operators."""
    import oracle_lib
    orc = oracle_lib.load()
    ref_crc = oracle_lib.load_ref_crc32()
    crc_fn = ref_crc if ref_crc is not None else orc.oracle_crc32_braid
    n = host_view.size
    ptr = host_view.ctypes.data
    pair, ta, tc = [], [], []
    a = c = 0
    for _ in range(reps):
        t0 = time.perf_counter()
        a = orc.oracle_adler32(1, ptr, n)
        t1 = time.perf_counter()
        c = crc_fn(0, ptr, n)
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tc.append(t2 - t1)
        pair.append(t2 - t0)
    gb = n / 1e9
    T = host_threads()
    cuts = [n * k // T for k in range(T + 1)]
    part = [None] * T

    try:
        cpus = sorted(os.sched_getaffinity(0))
    except AttributeError:
        cpus = []

    def work(k):
        if cpus:                                             # one thread per core, pinned
            try:
                os.sched_setaffinity(0, {cpus[k % len(cpus)]})
            except OSError:
                pass
        p, ln = ptr + cuts[k], cuts[k + 1] - cuts[k]
        part[k] = (orc.oracle_adler32(1, p, ln), crc_fn(0, p, ln), ln)

    multi = []
    am = cm = 0
    for _ in range(reps):
        ths = [threading.Thread(target=work, args=(k,)) for k in range(T)]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        am, cm = part[0][0], part[0][1]
        for k in range(1, T):
            am = zr.rocm.adler32_combine(am, part[k][0], part[k][2])
            cm = zr.rocm.crc32_combine(cm, part[k][1], part[k][2])
        multi.append(time.perf_counter() - t0)
    assert (am, cm) == (a, c), "T-thread slices + combine differ from the one-thread value"
    crc_name = "reference crc32_braid_c.c via oracle/_ref" if ref_crc is not None else "oracle port of crc32_braid_c.c"
    system = system_zlib_probe(ptr, n, reps)
    if system is not None:
        assert system.pop("checks") == [a, c], "the system zlib disagrees with the checker"
    return {
        "value": round(gb / statistics.median(pair), 3),
        "unit": "GB/s",
        "cores": 1,
        "kind": "port",
        "sample": ("%d MiB of the step's own buffer, %d reps, median; one thread runs adler32 (oracle port of "
                   "adler32_c.c) then crc32 (%s)" % (n >> 20, reps, crc_name)),
        "adler32_GBps": round(gb / statistics.median(ta), 3),
        "crc32_GBps": round(gb / statistics.median(tc), 3),
        "multi": {"value": round(gb / statistics.median(multi), 3), "unit": "GB/s", "cores": T,
                  "sample": "same buffer cut into %d contiguous slices, one thread each (all host cores this process "
                            "may use, pinned), adler32 then crc32 per slice, folded with adler32_combine / crc32_combine; median of %d" % (T, reps)},
        "system_zlib": system,
        "reference_container": REFERENCE_CONTAINER,
    }, (a, c)


def pmc_traffic(kernel, nbytes):
    """HBM bytes per launch of `kernel` from the committed PMC passes (profiles/r*_pmc_summary.json: separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same command, gfx950 FETCH_SIZE x2 correction applied).
    Counters cannot be read live from inside the timed run; null when no summary matches this workload."""
    best = None
    pdir = os.path.join(ROOT, "profiles")
    for name in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
        if "_pmc_summary" in name and name.endswith(".json"):      # later files (sorted) win: newest build last
            try:
                doc = json.load(open(os.path.join(pdir, name)))
            except ValueError:
                continue
            for kname, k in doc.get("kernels", {}).items():
                if kname.startswith(kernel) and doc.get("bytes_per_launch_algorithmic") == nbytes \
                        and "hbm_bytes_per_launch_corrected" in k:
                    best = {"bytes": k["hbm_bytes_per_launch_corrected"], "source": "profiles/" + name}
    return best


def copy_ceiling(torch, buf):
    """measured device-copy ceiling of this box: a plain device-to-device copy of the step's
    buffer, 2N bytes of HBM traffic per copy, timed with events after its own warm-up"""
    dst = torch.empty_like(buf)
    for _ in range(20):
        dst.copy_(buf)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        dst.copy_(buf)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / 20
    del dst
    return 2 * buf.numel() / 1e9 / (ms / 1e3)


def run_streams(args, zr, par, torch, dist, dev, world, rank, rehearse, steps, warmup, dump=None):
    """BASELINE.json configs[4]: `--streams` independent 1 MiB streams, level-1 class, sharded over the ranks
    (strong scaling: the total is fixed).  Step = every rank compresses its shard (LZ77 parse + static-Huffman emit)
    and the {clen, adler32, ulen} table is all-gathered (RCCL, 24 bytes per stream) and prefix-summed on every rank.
    Returns the `streams` object (rank 0) or None; `dump` (a directory, rank 0) receives the last step's table."""
    import zlib

    import numpy as np
    import synth
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    each, distinct = 1 << 20, 96
    first, count = par.shard_streams(args.streams, world, rank)
    # stream i = slice (i mod 96) of a 96 MiB six-class mix (seed 0x5EED0005): every rank can rebuild any stream
    base = synth.silesia_like(distinct << 20, seed=0x5EED0005, seg_bytes=1 << 20)
    d_base = torch.from_numpy(base).to(dev).view(distinct, each)
    idx = torch.arange(first, first + count, device=dev) % distinct
    src = d_base[idx].reshape(-1).contiguous() if count else torch.zeros(16, dtype=torch.uint8, device=dev)
    del d_base
    # Few streams per GPU (N > 1: the job is fixed, the shard shrinks) would leave most of a GPU idle: one workgroup per
    # stream, eight per CU.  Then every stream is compressed as pigz does it (pigz.c: blocks primed with the 32 KiB before
    # them, each closed by a sync-flush marker, concatenated): `blocks` blocks per stream keep >= 2048 jobs on the GPU.
    blocks = 1
    while count and count * blocks < 2048 and blocks < 8:
        blocks *= 2
    blk = each // blocks
    offs = [i * each + b * blk for i in range(count) for b in range(blocks)]
    dicts = [min(32768, b * blk) for i in range(count) for b in range(blocks)]
    flg = [(dfl.BLOCK_NOT_FINAL | dfl.BLOCK_SYNC_FLUSH) if b + 1 < blocks else 0 for i in range(count) for b in range(blocks)]
    batch = dfl.QuickBatch(src, offs, [blk] * (count * blocks), dict_len=dicts, flags=flg)
    ulen = torch.full((count,), each, dtype=torch.int64, device=dev)

    def stream_rows():
        """{clen, adler32} per STREAM from the per-block rows: lengths add, Adler-32 values combine (adler32_combine_,
        adler32.c:32-54, vectorised over the streams: one step per block)"""
        res = batch.results.to(torch.int64) & 0xffffffff
        if blocks == 1:
            return res[:, 0], res[:, 1]
        r = res.view(count, blocks, 2)
        a, bsum = r[:, 0, 1] & 0xffff, r[:, 0, 1] >> 16
        for k in range(1, blocks):
            a2, b2 = r[:, k, 1] & 0xffff, r[:, k, 1] >> 16
            bsum = (bsum + b2 + (blk % 65521) * ((a + 65520) % 65521)) % 65521
            a = (a + a2 + 65520) % 65521
        return r[:, :, 0].sum(1), a | (bsum << 16)
    per = (args.streams + world - 1) // world
    padded = torch.zeros((per, 3), dtype=torch.int64, device=dev)
    gathered = torch.zeros((world * per * 3,), dtype=torch.int64, device=dev)
    state = {}

    def exchange():
        if count:
            padded[:count, 0], padded[:count, 1] = stream_rows()
            padded[:count, 2] = ulen
        if world > 1 and not rehearse:
            dist.all_gather_into_tensor(gathered, padded.view(-1))       # RCCL, 24 bytes per stream
            table = gathered.view(world * per, 3)[:args.streams]
        elif world > 1:
            table = par.gather_rows(padded.view(-1).cpu()).view(world * per, 3)[:args.streams].to(dev)
        else:
            table = padded[:args.streams]
        state["table"] = table
        state["offsets"] = torch.cumsum(table[:, 0], 0) - table[:, 0]    # where each stream lands in one archive

    def step():
        batch.run()
        exchange()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(max(1, warmup)):
        step()
    fence()
    zr.rocm.lib().zng_rocm_trace_stride(1)
    zr.trace_begin(steps)
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    kernel_ms = zr.trace_end(steps)
    t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearse else dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()
    table = state["table"].cpu()
    if dump and rank == 0:
        dump_outputs(dump, {"streams_table": table.numpy()})
    # the exchange by itself (latency bound: tens of KiB), reported separately as SURVEY.md 8e asks
    fence()
    ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ea.record()
    for _ in range(10):
        exchange()
    eb.record()
    eb.synchronize()
    exchange_us = ea.elapsed_time(eb) / 10 * 1e3
    # parity on this rank: first and last local stream round-trip through an independent inflater, every local
    # Adler-32 row equals that of its slice
    res = batch.results.cpu()
    adlers = [zlib.adler32(base[k * each:(k + 1) * each].tobytes()) for k in range(distinct)]
    if count:
        s_clen, s_adler = (v.cpu() for v in stream_rows())
    for i in range(count):
        assert int(s_adler[i]) == adlers[(first + i) % distinct], "adler32 row %d" % (first + i)
    for i in ([0, count - 1] if count else []):
        k = (first + i) % distinct
        joined = b"".join(batch.compressed(i * blocks + b, res) for b in range(blocks))     # the stream = its blocks in order
        assert len(joined) == int(s_clen[i])
        assert zlib.decompressobj(-15).decompress(joined) == base[k * each:(k + 1) * each].tobytes()
    # ... and back, on the device: this rank's compressed streams through zng_rocm_inflate_streams_dev (one wavefront per
    # stream: block headers, table build, Huffman decode and copies), compared with the plaintext on the device
    inf = importlib.import_module("zlib-ng_amd.inflate")
    back_ms, back_kernel_ms = float("nan"), float("nan")
    if count:
        plain = torch.empty(count * each + 64, dtype=torch.uint8, device=dev)
        clens = [int(v) for v in s_clen]
        if blocks == 1:
            comp, comp_off = batch.dst, batch.out_off
        else:                                   # lay every stream's blocks end to end (not timed)
            comp = torch.cat([batch.dst[batch.out_off[j]:batch.out_off[j] + int(res[j, 0])] for j in range(count * blocks)] +
                             [torch.zeros(16, dtype=torch.uint8, device=dev)])
            comp_off, at = [], 0
            for c in clens:
                comp_off.append(at)
                at += c
        ib = inf.InflateDevBatch(comp, comp_off, clens, plain, [i * each for i in range(count)], [each] * count)
        ib.run()
        fence()
        reps = 3
        zr.trace_begin(reps)
        t0 = time.perf_counter()
        for _ in range(reps):
            ib.run()
        fence()
        back_ms = (time.perf_counter() - t0) / reps * 1e3
        km = zr.trace_end(reps)
        back_kernel_ms = statistics.mean(km) if km else float("nan")
        rows = ib.results.cpu()
        assert bool((rows[:, 2] == 1).all()) and bool((rows[:, 0] == each).all()) and rows[:, 1].tolist() == clens
        assert torch.equal(plain[:count * each], src[:count * each]), "device inflate differs from the plaintext"
        del plain, ib
    tb = torch.tensor([back_ms if count else 0.0], dtype=torch.float64, device="cpu" if rehearse else dev)
    if world > 1:
        dist.all_reduce(tb, op=dist.ReduceOp.MAX)
    back_ms = tb.item()
    if rank != 0:
        return None
    total_in = args.streams * each
    total_out = int(table[:, 0].sum())
    assert int(table[:, 2].sum()) == total_in and int(state["offsets"][-1] + table[-1, 0]) == total_out
    k_ms = statistics.mean(kernel_ms) if kernel_ms else float("nan")
    local_bytes = count * each + int(res[:, 0].to(torch.int64).sum())
    layout = "one static block per stream" if blocks == 1 else \
        "%d blocks of %d KiB per stream, each primed with the 32 KiB before it and closed by a sync-flush marker (pigz), " \
        "the blocks of a stream concatenate into its deflate stream" % (blocks, blk >> 10)
    out = {
        "workload": "configs[4]: %d independent 1 MiB streams, deflate level-1 class (static Huffman), sharded %d-way, "
                    "{clen, adler32, ulen} table all-gathered" % (args.streams, world),
        "value": round(total_in / 1e9 / (elapsed / steps), 2), "unit": "GB/s", "scaling": "strong",
        "n_gpus": world, "steps": steps, "warmup": max(1, warmup), "ms_per_step": round(elapsed / steps * 1e3, 3),
        "streams_per_gpu": count, "blocks_per_stream": blocks, "layout": layout, "ratio": round(total_in / total_out, 3),
        "exchange_us": round(exchange_us, 1),
        "exchange": "all_gather of %d B per rank (24 B per stream) + exclusive scan of clen on every rank; inside "
                    "ms_per_step, also timed alone here" % (per * 24),
        "parallelism": "streams/%d+allgather(24B/stream)" % world, "rehearsal_same_gpu": rehearse,
        "roofline": {"bound": "hbm", "kernel": "zr::deflate_quick_kernel (level-1 class: LZ77 parse with the static-Huffman emit fused in, DESIGN.md 3.5)",
                     "achieved": round(local_bytes / 1e9 / (k_ms / 1e3), 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(local_bytes / 1e9 / (k_ms / 1e3) / HBM_PEAK_GBPS, 4), "traffic": None,
                     "algorithmic_bytes_per_launch": local_bytes, "avg_kernel_ms": round(k_ms, 3)},
    }
    out["inflate_back"] = {
        "workload": "the same %d streams, as compressed above, decoded on the device (zng_rocm_inflate_streams_dev) and "
                    "compared with the plaintext on the device" % args.streams,
        "value": round(total_in / 1e9 / (back_ms / 1e3), 2), "unit": "GB/s of output", "ms": round(back_ms, 3),
        "kernel_ms_rank0": round(back_kernel_ms, 3), "bit_exact": True,
        "roofline": {"bound": "hbm", "kernel": "zr::inflate_streams_kernel (one wavefront per stream; scalar-issue bound, DESIGN.md 3.8)",
                     "achieved": round(local_bytes / 1e9 / (back_kernel_ms / 1e3), 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(local_bytes / 1e9 / (back_kernel_ms / 1e3) / HBM_PEAK_GBPS, 4), "traffic": None,
                     "algorithmic_bytes_per_launch": local_bytes, "avg_kernel_ms": round(back_kernel_ms, 3)},
        "reference_container_GBps": REFERENCE_CONTAINER["inflate_out_GBps"]}
    if not args.no_cpu:
        t0 = time.perf_counter()
        done = 0
        while time.perf_counter() - t0 < 8 and done < count:
            zlib.compress(base[(done % distinct) * each:(done % distinct + 1) * each].tobytes(), 1)
            done += 1
        dt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(done * each / 1e9 / dt, 4), "unit": "GB/s", "cores": 1, "kind": "port",
                               "sample": "%d of this rank's streams through CPython zlib level 1 (classic zlib 1.2.11, an "
                                         "independent codec: zlib-ng itself cannot be built under the round rules), one "
                                         "thread" % done,
                               "reference_container_GBps": REFERENCE_CONTAINER["deflate_level1_GBps"]}
    del batch, src
    torch.cuda.empty_cache()
    return out


def run_single_stream_legs(args, zr, torch, dist, dev, world, rank):
    """The two single-stream members of the metric (BASELINE.json configs[2] and [3]): deflate level 6 of one 256 MiB
    stream and raw inflate of it.  A single deflate / inflate stream does not shard over GPUs (32 KiB of history):
    at N > 1 every rank runs its own replica ("replicas only") and the values are sums.
    deflate: plaintext resident in HBM -> raw stream in HBM (zng_rocm_deflate_dev, includes its host synchronisation).
    inflate: host stream -> plaintext in HBM, host decode on the threads this rank may use (zng_rocm_inflate_raw_threads),
    and the same on one thread."""
    import zlib

    import synth
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    inf = importlib.import_module("zlib-ng_amd.inflate")
    n = 256 << 20
    plain = synth.silesia_like(n, seed=0x5EED0003)
    src = torch.from_numpy(plain).to(dev)
    dst, clen = dfl.deflate_dev(src, level=6)                     # warm-up: allocates the per-stream scratch
    torch.cuda.synchronize()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, reps):
        fence()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        fence()
        dt = torch.tensor([(time.perf_counter() - t0) / reps], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        return dt.item()

    t_def = timed(lambda: dfl.deflate_dev(src, level=6), 3)
    comp = dst[:clen].cpu().numpy().tobytes()
    d = zlib.decompressobj(-15)                                  # validity: an independent inflater restores the first 8 MiB
    assert d.decompress(comp[:4 << 20], 8 << 20) == plain[:8 << 20].tobytes()
    hs = inf.HostStream(comp)
    out = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    T = max(1, host_threads() // world)
    inf.inflate_raw_threads(hs, out, nthreads=T)                 # warm-up: the pooled pinned arrays
    res = {}

    def run_threads():
        res["rc"] = inf.inflate_raw_threads(hs, out, nthreads=T)
    t_inf = timed(run_threads, 3)
    assert res["rc"][:2] == (1, n) and torch.equal(out[:n], src), "inflate output differs from the plaintext"
    parts = zr.lib().zng_rocm_inflate_threads_last_parts()
    t_inf1 = timed(lambda: inf.inflate_raw_threads(hs, out, nthreads=1), 1)
    # the same stream, already in device memory, decoded on the device alone (zng_rocm_inflate_large_dev): block starts found
    # by a device kernel, one wavefront per part, the host only sorts candidates and walks the chain
    d_comp = dst[:clen].contiguous()
    out.zero_()
    inf.inflate_large_dev(d_comp, out)
    big = {}

    def run_large():
        big["rc"] = inf.inflate_large_dev(d_comp, out)
    t_large = timed(run_large, 3)
    assert big["rc"][:3] == (1, n, clen) and torch.equal(out[:n], src), "device inflate output differs from the plaintext"
    del src, dst, out, d_comp
    torch.cuda.empty_cache()
    if rank != 0:
        return None
    gb = n / 1e9
    return {
        "deflate_lvl6": {"workload": "configs[3]: deflate level-6 class of one 256 MiB Silesia-like stream per GPU, device resident",
                         "value": round(world * gb / t_def, 2), "unit": "GB/s of input", "ms_per_stream": round(t_def * 1e3, 2),
                         "ratio": round(n / clen, 3), "scaling": "replicas only" if world > 1 else "single",
                         "reference_container_GBps": REFERENCE_CONTAINER["deflate_level6_GBps"]},
        # configs[2]: the stream is resident in HBM when the timed region starts (the bench contract), so the figure is the
        # device path; the host-pointer path (token decode on host threads, PCIe for the tokens) is reported beside it
        "inflate": {"workload": "configs[2]: raw inflate of that level-6 stream (%.1f MiB, resident in HBM) into HBM, bit-exact vs the "
                                "plaintext; zng_rocm_inflate_large_dev: block starts found on the device, one wavefront per part, "
                                "symbols resolved by the context chain; host: sort + chain walk on 1 thread" % (clen / 2**20),
                    "value": round(world * gb / t_large, 2), "unit": "GB/s of output", "ms_per_stream": round(t_large * 1e3, 2),
                    "in_GBps": round(world * clen / 1e9 / t_large, 2), "parts": big["rc"][3], "host_threads": 1,
                    "host_decode": {"what": "the same stream handed over as a HOST buffer to zng_rocm_inflate_raw_threads: token decode on "
                                            "%d host threads cut at found block boundaries, tokens over PCIe, device resolve; with ONE "
                                            "thread the call copies the stream up and decodes it on the device (PCIe inclusive)" % T,
                                    "GBps_of_output": round(world * gb / t_inf, 2), "ms_per_stream": round(t_inf * 1e3, 2),
                                    "host_threads": T, "parts_joined": parts, "one_host_thread_GBps": round(gb / t_inf1, 2)},
                    "scaling": "replicas only" if world > 1 else "single",
                    "reference_container_GBps": REFERENCE_CONTAINER["inflate_out_GBps"]},
    }


def emit(line):
    """the ONE JSON line goes to the process's real stdout; everything else any library prints there (RCCL's
    version banner at communicator creation, for one) was pointed at stderr when main() started"""
    os.write(_REAL_STDOUT, (json.dumps(line) + "\n").encode())


_REAL_STDOUT = 1


def dump_outputs(dirname, arrays):
    """--dump-outputs: every array as dirname/<name>.npy in float64 (u32 / i64 values up to 2^53 stay exact)"""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), np.asarray(a, dtype=np.float64))


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(n_ranks, argv):
    """`python bench.py --gpus N` (N > 1) outside any launcher: start the N ranks as ONE child process tree, one rank per
    GPU -- the many-stream model of the reference (test/pigz/CMakeLists.txt:123-200: independent workers, one result
    table).  Runs before this process has imported torch or made any HIP call (a process that has initialised the GPU
    must never exec or fork into another GPU program); the parent only waits, the child's stdout (rank 0's ONE JSON
    line) is inherited, the exit code is the launcher's."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, host_threads() // n_ranks)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def main():
    global _REAL_STDOUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shard-mib", type=int, default=SHARD_BYTES >> 20)
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything besides the top-level line: single-checksum kernel rates, "
                         "device-copy ceiling, cpu_baseline, and (default workload `all`) the streams / deflate_lvl6 / "
                         "inflate legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline legs")
    ap.add_argument("--settle", type=int, default=SETTLE_LAUNCHES, help="untimed launches in front of the warm-up (disclosed in the line)")
    ap.add_argument("--workload", choices=("all", "checksum", "streams"), default=None,
                    help="all = BASELINE.json configs[1] as the top-level line (the driver's contract) plus the "
                         "configs[4] `streams` object and the single-stream legs (implies --full); checksum = the "
                         "top-level line only; streams = configs[4] only, printed as the line.  Default: all with "
                         "--full, checksum without")
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-steps", type=int, default=0, help="timed steps of the streams leg (0 = min(steps, 6))")
    ap.add_argument("--launch-only", action="store_true",
                    help="every rank prints {rank, world, local_rank} as one JSON line and exits: exercises the launcher "
                         "without a GPU (tests/test_bench_launch.py)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.workload is None:
        args.workload = "all" if args.full else "checksum"
    full = args.full or args.workload == "all"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args.gpus, sys.argv[1:]))       # nothing above this line imports torch or touches HIP
    if args.gpus > 1 and world != args.gpus:
        sys.exit("--gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    if args.launch_only:
        # one write per rank: lines of different ranks must not interleave on the shared stdout
        os.write(1, (json.dumps({"launch_only": True, "rank": rank, "world": world, "local_rank": local_rank,
                                 "master": "%s:%s" % (os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT"))}) + "\n").encode())
        return
    sys.stdout.flush()
    _REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)

    import numpy as np  # noqa: F401
    import torch
    import torch.distributed as dist

    # ZNG_BENCH_REHEARSE=1: every rank on cuda:0 with the gloo backend -- lets the N>1 control flow be
    # rehearsed on a one-GPU box (RCCL refuses two ranks on one device); numbers from it mean nothing.
    rehearse = os.environ.get("ZNG_BENCH_REHEARSE") == "1"
    # ZNG_BENCH_FORCE_DIST=1: take the N > 1 code path (RCCL all-gather on the side stream, combine_rows) with a
    # one-rank process group -- the way to exercise that path on a one-GPU box
    force_dist = os.environ.get("ZNG_BENCH_FORCE_DIST") == "1" and world == 1
    if rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1 or force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if force_dist:
            os.environ.setdefault("MASTER_PORT", "29531")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if rehearse:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=dev)

    zr = importlib.import_module("zlib-ng_amd")      # raises if libzng_rocm.so is missing: no fallback
    zr.init(local_rank)
    par = importlib.import_module("zlib-ng_amd.parallel")
    stream_steps = args.stream_steps or max(1, min(args.steps, 6))
    stream_warm = max(1, min(args.warmup, 2))

    if args.workload == "streams":
        s = run_streams(args, zr, par, torch, dist, dev, world, rank, rehearse, args.steps, args.warmup,
                        dump=args.dump_outputs)
        if rank == 0:
            line = {"metric": METRIC, "value": s["value"], "unit": "GB/s", "n_gpus": world, "steps": args.steps,
                    "warmup": max(1, args.warmup), "ms_per_step": s["ms_per_step"], "higher_is_better": True,
                    "scaling": "strong", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
                    "config": {"workload": s["workload"], "streams_per_gpu": s["streams_per_gpu"], "ratio": s["ratio"],
                               "parallelism": s["parallelism"], "rehearsal_same_gpu": rehearse},
                    "roofline": s["roofline"], "exchange_us": s["exchange_us"]}
            if "cpu_baseline" in s:
                line["cpu_baseline"] = s["cpu_baseline"]
            line["inflate_back"] = s["inflate_back"]
            emit(line)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    n = args.shard_mib << 20
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED + rank)
    buf = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=gen)
    out = torch.zeros(2, dtype=torch.int32, device=dev)
    # N > 1: each rank's {adler, crc, len} row (16 bytes, zng_rocm_check_row) is all-gathered and folded in rank order
    # by ONE device launch pair (zng_rocm_combine_rows_dev).  The exchange of step k runs on a side stream while the
    # main stream is already in step k+1's checksum kernel: the collective (latency bound: 16 bytes per rank over
    # xGMI) never sits on the critical path.  Rows rotate through k_slots buffers; a slot is reused only after the
    # side stream has released it.  The checksum kernel writes its two words straight into the row.
    multi = world > 1 or force_dist
    k_slots = 8
    rows_local = [torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(k_slots)]
    for r in rows_local:
        lo = n & 0xffffffff
        r[2] = lo if lo < (1 << 31) else lo - (1 << 32)
        r[3] = n >> 32
    rows_all = [torch.zeros(world * 4, dtype=torch.int32, device=dev) for _ in range(k_slots)]
    totals = [torch.zeros(2, dtype=torch.int32, device=dev) for _ in range(k_slots)]
    side = torch.cuda.Stream(device=dev, priority=-1)    # its own hardware queue: must not share the main one
    # Cross-stream synchronisation is per GROUP of k_group steps, not per step: every step still has its own all-gather
    # and its own combine, but an event-record packet in front of every checksum launch costs ~10 us of launch gap
    # (traced), so the exchanges of a group are issued together behind one event.
    k_group = 4
    n_groups = k_slots // k_group
    produced = [torch.cuda.Event() for _ in range(n_groups)]
    released = [torch.cuda.Event() for _ in range(n_groups)]
    state = {"k": 0, "last": 0}

    # Host cost matters as much as device cost here: a step is 0.18 ms of kernel, and every Python-side stream switch
    # or tensor op in the loop is tens of microseconds.  So inside the loop torch's *current* stream IS the exchange
    # stream (the collective and the combine pick it up implicitly) and the checksum kernel is launched on `main`
    # explicitly -- no per-step stream context, no tensor arithmetic.
    main_stream = torch.cuda.current_stream()
    # ZNG_BENCH_SIMPLE_EXCHANGE=1: no second stream -- kernel, all-gather and combine in order on the main stream
    # (the plain form of the same step; kept as a switch so the overlapped form can be compared against it)
    simple = os.environ.get("ZNG_BENCH_SIMPLE_EXCHANGE") == "1"

    # ---- settle phase: untimed, disclosed (`settle_launches`) --------------------------------------------------
    # At least args.settle launches, then batches of 200 (~35 ms) until fifteen in a row (~0.5 s) bring no batch that is more
    # than 0.1 % faster than the best so far -- or 15000 launches (2.5 s).  Measured on the MI355X boxes: started within a few
    # seconds of a heavy GPU job (the test suite), the same kernel runs 4-5 % slower for about two seconds and creeps up --
    # 0.79 of peak behind a 300- or 1000-launch settle, 0.825 behind 12000, 0.828 behind 600 after a 12 s pause; on an idle
    # box 300 are enough.  The count is disclosed in the line (`settle_launches`).
    settled = 0
    for _ in range(args.settle):
        zr.adler32_crc32_dev(buf, out, adler=1, crc=0)
    settled += args.settle
    torch.cuda.synchronize()
    best, stale = None, 0
    while settled < 15000 and stale < 15:
        t0 = time.perf_counter()
        for _ in range(200):
            zr.adler32_crc32_dev(buf, out, adler=1, crc=0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        settled += 200
        if best is None or dt < 0.999 * best:
            best, stale = dt if best is None else min(best, dt), 0
        else:
            best, stale = min(best, dt), stale + 1

    if multi and not rehearse and not simple:
        torch.cuda.set_stream(side)
        # the checksum grid is one workgroup per CU for the whole pass: leave a few CUs to the exchange stream, so
        # that the collective's workgroups do not have to displace one the pass then waits for
        zr.reserve_cus(int(os.environ.get("ZNG_BENCH_RESERVE_CUS", "4")))

    def exchange(group, count):
        """the exchanges of `count` finished steps of this group: one all-gather + one combine each"""
        produced[group].record(main_stream)
        side.wait_event(produced[group])
        for j in range(count):
            slot = group * k_group + j
            par.gather_check_rows(rows_local[slot], rows_all[slot])      # RCCL all-gather on the exchange stream, 16 B per rank
            zr.combine_rows_dev(rows_all[slot], world, totals[slot], stream=side)
        released[group].record(side)

    def step():
        if not multi:
            zr.adler32_crc32_dev(buf, out, adler=1, crc=0)
            return
        slot = state["k"] % k_slots
        group, pos = divmod(slot, k_group)
        row = rows_local[slot]
        if pos == 0 and state["k"] >= k_slots and not rehearse and not simple:
            main_stream.wait_event(released[group])      # the exchange stream is done with this group's slots
        zr.adler32_crc32_dev(buf, row, adler=1, crc=0, stream=main_stream)       # row[0:2] <- {adler, crc}
        state["last"] = slot
        state["k"] += 1
        if rehearse:
            # gloo has no device tensors: same payload and fold, synchronously through the host
            g = par.gather_check_rows(row.cpu()).to(dev)
            zr.combine_rows_dev(g, world, totals[slot], stream=main_stream)
        elif simple:
            par.gather_check_rows(row, rows_all[slot])   # current stream = main
            zr.combine_rows_dev(rows_all[slot], world, totals[slot], stream=main_stream)
        elif pos == k_group - 1:
            exchange(group, k_group)

    def flush():
        """exchanges of a partly filled group (step counts that are not a multiple of k_group)"""
        pending = state["k"] % k_group
        if multi and not rehearse and not simple and pending:
            exchange((state["k"] % k_slots) // k_group, pending)
            state["k"] += k_group - pending              # the next step starts a fresh group

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    flush()
    fence()
    stride = TRACE_STRIDE if args.steps >= 4 * TRACE_STRIDE else 1
    zr.rocm.lib().zng_rocm_trace_stride(stride)
    zr.trace_begin(args.steps)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    flush()
    fence()
    elapsed = time.perf_counter() - t0
    kernel_ms = zr.trace_end(args.steps)
    zr.rocm.lib().zng_rocm_trace_stride(1)

    t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearse else dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()

    torch.cuda.set_stream(main_stream)
    last = state["last"] if multi else 0
    result = [v & 0xffffffff for v in (rows_local[last][0:2] if multi else out).tolist()]
    if multi:
        # the on-device ordered combine must equal the host fold of the gathered rows
        mine = rows_local[last]
        g = par.gather_check_rows(mine.cpu()) if rehearse else par.gather_check_rows(mine)
        rows = par.check_rows_to_list(g.cpu())
        folded = par.fold_checksums(rows)
        got_total = [v & 0xffffffff for v in totals[last].tolist()]
        assert got_total == [folded[0], folded[1]], (got_total, folded)
        assert rows[rank][:2] == result and all(r[2] == n for r in rows)
        zr.reserve_cus(0)
    if args.dump_outputs and rank == 0:
        arrays = {"checksums": result}
        if multi:
            arrays["combined"] = got_total
        dump_outputs(args.dump_outputs, arrays)
    # --full: separate single-checksum timings and the device-copy ceiling (outside the timed region, informational)
    extra = {}
    singles = (("adler32", lambda: zr.adler32_dev(buf, out)), ("crc32", lambda: zr.crc32_dev(buf, out))) if full else ()
    for name, fn in singles:
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        zr.trace_begin(20)
        for _ in range(20):
            fn()
        ms = zr.trace_end(20)
        extra[name + "_kernel_GBps"] = round(n / 1e9 / (statistics.mean(ms) / 1e3), 1)
    measured_copy = copy_ceiling(torch, buf) if rank == 0 and full else None

    line = None
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = world * n / 1e9 / (elapsed / args.steps)
        k_avg_ms = statistics.mean(kernel_ms) if kernel_ms else float("nan")
        achieved = n / 1e9 / (k_avg_ms / 1e3)
        traffic = pmc_traffic("zr::stream_kernel<true, true, false", n) or {}
        line = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "settle_launches": settled,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "config": {
                "workload": "configs[1]: crc32 + adler32 over a %d MiB synthetic buffer per GPU, HBM-resident, "
                            "fused single pass + on-device combine" % (n >> 20),
                "bytes_per_gpu": n,
                "parallelism": ("shard%d+allgather(16B/rank, side stream, overlapped with the next step)+ordered-combine" % world)
                if multi else "single",
                "checksums": ["%08x" % result[0], "%08x" % result[1]],
                "rehearsal_same_gpu": rehearse,
                "settle": "%d untimed launches of the same kernel before the %d warm-up steps (clock settle, not part of "
                          "any timed figure)" % (settled, args.warmup),
            },
            "roofline": {
                "bound": "hbm",
                "kernel": "zr::stream_kernel<adler,crc> (fused pass)",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBPS, 4),
                "traffic": traffic.get("bytes"),
                "traffic_source": traffic.get("source"),
                "algorithmic_bytes_per_launch": n,
                "avg_kernel_ms": round(k_avg_ms, 5),
                "launches_timed": len(kernel_ms),
                "launches_sampled_every": stride,
            },
        }
        if measured_copy is not None:
            line["roofline"].update({
                "measured_copy_GBps": round(measured_copy, 1),
                "frac_of_measured_copy": round(achieved / measured_copy, 4),
                "measured_copy": "torch device-to-device copy of the same %d MiB buffer, 2N bytes per copy, on this GPU" % (n >> 20),
            })
        line.update(extra)
        if full and not args.no_cpu:
            host = buf.cpu().numpy()
            cb, (a, c) = cpu_baseline(host, zr)
            assert [a, c] == result, "GPU result differs from the CPU checker: %r vs %r" % (result, [a, c])
            line["cpu_baseline"] = cb
            del host

    if args.workload == "all":
        del buf
        torch.cuda.empty_cache()
        s = run_streams(args, zr, par, torch, dist, dev, world, rank, rehearse, stream_steps, stream_warm)
        if rank == 0:
            line["streams"] = s
        legs = run_single_stream_legs(args, zr, torch, dist, dev, world, rank)
        if rank == 0:
            line.update(legs)
    if rank == 0:
        emit(line)

    if world > 1 or force_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
