"""A BATCH of large raw deflate streams inflated on the device in one set of launches per round
(zng_rocm_inflate_large_streams_dev): the finder, the part launch, the compaction and the resolve of
zng_rocm_inflate_large_ex_dev run once over the parts of all streams of a round.  The loop replaced is inflate_fast
(inffast_tpl.h:151-298) with the headers around it (inflate.c:735-917), per stream.  Oracle: the plaintext for the bytes;
for every other field the one-stream call zng_rocm_inflate_large_ex_dev on the same job in a call of its own (the parity
contract: status; on 1 also out_len, in_used and the bytes; on -3 also the message)."""
import importlib
import threading
import zlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), importlib.import_module("zlib-ng_amd.deflate")


def _raw(plain, level, zdict=None, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy, zdict) if zdict else \
        zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(plain) + c.flush()


def _dev(torch, data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _own6(torch, dfl, plain):
    c, n = dfl.deflate_dev(_dev(torch, plain), level=6)
    return c[:n].cpu().numpy().tobytes()


def _quick(torch, dfl, plain):
    n = len(plain)
    src = torch.zeros((n + 15) & ~15, dtype=torch.uint8, device="cuda")
    src[:n] = _dev(torch, plain)
    q = dfl.QuickBatch(src, [0], [n])
    q.run()
    torch.cuda.synchronize()
    return q.compressed(0)


class Job:
    """one stream of a batch: compressed bytes, the plaintext a clean decode gives (or None), optional history, dst_cap"""

    def __init__(self, torch, name, comp, plain, window=None, cap=None, odd=0):
        self.name, self.comp, self.plain = name, bytes(comp), plain
        self.src = _dev(torch, comp)
        self.window = None if window is None else _dev(torch, window)
        self.cap = (len(plain) if plain is not None else 8 * MiB) if cap is None else cap
        self.odd = odd                                    # the destination's address modulo 16

    def dst(self, torch, guard=64):
        """(whole buffer, the dst_cap bytes handed to the library) -- 0xAB everywhere"""
        whole = torch.full((16 + self.cap + guard,), 0xAB, dtype=torch.uint8, device="cuda")
        assert whole.data_ptr() % 16 == 0
        return whole, whole[self.odd:self.odd + self.cap]


def _alone(torch, inf, zr, job, subblock):
    """the reference: zng_rocm_inflate_large_ex_dev on this job in a call of its own"""
    whole, dst = job.dst(torch)
    st, n, used, parts = inf.inflate_large_dev(job.src, dst, window=job.window, subblock=subblock)
    msg = zr.rocm.lib().zng_rocm_last_error().decode() if st == -3 else None
    return st, n, used, parts, msg, whole, dst


def _run_batch(torch, inf, jobs, subblock, round_bytes=0, stream=None):
    bufs = [j.dst(torch) for j in jobs]
    torch.cuda.synchronize()
    rc, rows, rounds, launches = inf.inflate_large_streams_dev([j.src for j in jobs], [b[1] for b in bufs],
                                                               windows=[j.window for j in jobs], round_bytes=round_bytes,
                                                               subblock=subblock, stream=stream)
    return rc, rows, rounds, launches, bufs


def _check_parity(torch, jobs, rows, bufs, refs):
    for j, row, (whole, dst), ref in zip(jobs, rows, bufs, refs):
        st, n, used, msg, parts, _ = row
        rst, rn, rused, rparts, rmsg, rwhole, rdst = ref
        assert st == rst, (j.name, row, ref[:5])
        if st == 1:
            assert (n, used) == (rn, rused), (j.name, row, ref[:5])
            assert torch.equal(dst[:n], rdst[:n]), j.name
            if j.plain is not None:
                assert n == len(j.plain) and dst[:n].cpu().numpy().tobytes() == j.plain, j.name
        elif st == -3:
            assert msg == rmsg, (j.name, msg, rmsg)
        # nothing at or behind d_dst + dst_cap, nothing in front of d_dst
        assert int(whole[j.odd + j.cap:].min()) == 0xAB and (j.odd == 0 or int(whole[:j.odd].min()) == 0xAB), j.name
        if rparts > 0:                                    # what the one-stream call does on the device, the batch does too
            assert parts > 0, (j.name, row, ref[:5])


@pytest.fixture(scope="module")
def mixed(mods):
    """>= 12 jobs: writers CPython 1 / 6 / 9 and Z_FIXED, this library's level 6 and quick; 2 .. 32 MiB of plaintext; two
    jobs with history; destinations at odd addresses"""
    torch, inf, dfl = mods
    zr = importlib.import_module("zlib-ng_amd")
    spec = [("cpy1-8", 8, "c1"), ("cpy6-32", 32, "c6"), ("cpy9-4", 4, "c9"), ("fixed-6", 6, "cf"), ("own6-16", 16, "o6"),
            ("quick-4", 4, "oq"), ("cpy6-2", 2, "c6"), ("own6-2", 2, "o6"), ("cpy6-win32k-4", 4, "w32"),
            ("cpy6-win1000-3", 3, "w1k"), ("cpy1-2", 2, "c1"), ("quick-8", 8, "oq"), ("cpy6-5", 5, "c6")]
    jobs = []
    for k, (name, mib, kind) in enumerate(spec):
        plain = synth.silesia_like(mib * MiB + 977 * k, seed=0xBA7C4 + k).tobytes()
        window = None
        if kind == "c1":
            comp = _raw(plain, 1)
        elif kind == "c6":
            comp = _raw(plain, 6)
        elif kind == "c9":
            comp = _raw(plain, 9)
        elif kind == "cf":
            comp = _raw(plain, 6, strategy=zlib.Z_FIXED)
        elif kind == "o6":
            comp = _own6(torch, dfl, plain)
        elif kind == "oq":
            comp = _quick(torch, dfl, plain)
        else:
            window = plain[-32768:] if kind == "w32" else plain[-1000:]
            comp = _raw(plain, 6, zdict=window)
        jobs.append(Job(torch, name, comp, plain, window=window, odd=(1, 3, 7, 0, 5, 9, 15, 2)[k % 8]))
    refs = {sub: [_alone(torch, inf, zr, j, sub) for j in jobs] for sub in (False, True)}
    return jobs, refs


@pytest.mark.parametrize("subblock", [False, True])
def test_parity_with_the_one_stream_call_and_one_set_of_launches(mods, mixed, subblock):
    torch, inf, _ = mods
    jobs, refs = mixed
    assert len(jobs) >= 12
    rc, rows, rounds, launches, bufs = _run_batch(torch, inf, jobs, subblock)
    assert rc == 0
    _check_parity(torch, jobs, rows, bufs, refs[subblock])
    assert all(r[0] == 1 for r in rows), rows
    # the batch is a batch: one round, the part kernel launched once (twice with a rerun), more parts than jobs
    assert rounds == 1 and 1 <= launches <= 2, (rounds, launches)
    assert sum(r[4] for r in rows) > len(jobs), rows
    on_device = [r[3] > 0 for r in refs[subblock]]
    assert sum(on_device) >= (len(jobs) - 1 if subblock else 8), [(j.name, r[3]) for j, r in zip(jobs, refs[subblock])]
    if subblock:
        assert any(r[5] > 0 for r in rows), rows          # some parts began inside blocks


def test_rounds(mods, mixed):
    torch, inf, dfl = mods
    jobs, refs = mixed
    for subblock in (False, True):
        rc, rows, rounds, launches, bufs = _run_batch(torch, inf, jobs, subblock, round_bytes=4 * MiB)
        assert rc == 0
        _check_parity(torch, jobs, rows, bufs, refs[subblock])
        assert rounds > 1 and launches <= 2 * rounds, (rounds, launches)
    # 300 streams of 2 MiB of this library's level-6 class (ten different ones) in one round: the pattern finder alone
    plains = [synth.silesia_like(2 * MiB, seed=0x300 + k).tobytes() for k in range(10)]
    comps = [_own6(torch, dfl, p) for p in plains]
    srcs = [_dev(torch, c) for c in comps]
    want = [_dev(torch, p) for p in plains]
    n = 300
    dsts = [torch.zeros(2 * MiB, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    rc, rows, rounds, launches = inf.inflate_large_streams_dev([srcs[i % 10] for i in range(n)], dsts)
    assert rc == 0 and rounds == 1 and launches <= 2, (rc, rounds, launches)
    for i, row in enumerate(rows):
        assert row[:4] == (1, 2 * MiB, len(comps[i % 10]), None) and row[4] >= 4, (i, row)
        assert torch.equal(dsts[i], want[i % 10]), i


@pytest.mark.parametrize("subblock", [False, True])
def test_neighbours_of_trouble(mods, subblock):
    """damaged, short and extreme streams between regular ones: each gets what the one-stream call gives it, and the regular
    neighbours stay on the device"""
    torch, inf, dfl = mods
    zr = importlib.import_module("zlib-ng_amd")

    def plain(mib, k):
        return synth.silesia_like(mib * MiB, seed=0x7B0 + k).tobytes()

    regular = [Job(torch, "regular-%d" % k, _raw(plain(4, k), 6) if k % 2 else _own6(torch, dfl, plain(4, k)), plain(4, k), odd=k + 1)
               for k in range(5)]
    p = plain(4, 10)
    c = _raw(p, 6)
    hdr = bytearray(c)
    hdr[2] ^= 0x5A                                        # in the first block's dynamic header
    data = bytearray(c)
    data[len(c) // 2] ^= 0x10                             # inside block data
    small = plain(1, 11)[:100 << 10]
    fixed = plain(4, 12)
    zeros = bytes(64 * MiB)
    runs = plain(2, 13) + bytes(24 * MiB) + plain(2, 14)  # parts of a ratio far above 64: the rerun with 1032 : 1 slots
    trouble = [Job(torch, "truncated", c[:len(c) // 2], None, cap=len(p)),
               Job(torch, "flip-header", hdr, None, cap=len(p)),
               Job(torch, "flip-data", data, None, cap=len(p)),
               Job(torch, "garbage-behind", c + bytes(range(100)), p),
               Job(torch, "40KiB-stream", _raw(small, 6), small, odd=3),
               Job(torch, "fixed-only", _raw(fixed, 6, strategy=zlib.Z_FIXED), fixed),
               Job(torch, "cap-one-short", c, None, cap=len(p) - 1, odd=5),
               Job(torch, "zeros-64MiB", _raw(zeros, 6), zeros),
               Job(torch, "runs-of-zeros", _raw(runs, 6), runs, odd=7)]
    assert 30 << 10 < len(trouble[4].comp) < 128 << 10
    jobs = []
    for k, t in enumerate(trouble):                       # interleaved
        jobs.append(t)
        if k < len(regular):
            jobs.append(regular[k])
    refs = [_alone(torch, inf, zr, j, subblock) for j in jobs]
    rc, rows, rounds, launches, bufs = _run_batch(torch, inf, jobs, subblock)
    assert rc == 0 and rounds == 1 and launches <= 2, (rc, rounds, launches)
    _check_parity(torch, jobs, rows, bufs, refs)
    by_name = {j.name: r for j, r in zip(jobs, rows)}
    for j in regular:
        assert by_name[j.name][0] == 1 and by_name[j.name][4] > 0, (j.name, by_name[j.name])
    assert by_name["truncated"][0] == -5 and by_name["cap-one-short"][0] == -5
    assert by_name["garbage-behind"][:3] == (1, len(p), len(c))
    assert by_name["runs-of-zeros"][0] == 1 and by_name["runs-of-zeros"][4] > 0 and launches == 2, (by_name["runs-of-zeros"], launches)


@pytest.fixture(scope="module")
def singles(mods):
    """three streams that take the pass's different ways: plain, with history, and with parts of a ratio far above 64 (the
    runs-of-zeros job of test_neighbours_of_trouble, at its size: the second part launch is what it is here for)"""
    torch, _, _ = mods
    plain = synth.silesia_like(2 * MiB, seed=0x51A61E).tobytes()
    window = plain[-1000:]
    runs = synth.silesia_like(2 * MiB, seed=0x7B0 + 13).tobytes() + bytes(24 * MiB) + synth.silesia_like(2 * MiB, seed=0x7B0 + 14).tobytes()
    return [Job(torch, "cpy6-2", _raw(plain, 6), plain, odd=7),
            Job(torch, "cpy6-win1000-2", _raw(plain, 6, zdict=window), plain, window=window, odd=3),
            Job(torch, "runs-of-zeros", _raw(runs, 6), runs, odd=5)]


@pytest.mark.parametrize("subblock", [False, True])
def test_a_batch_of_one_is_the_one_stream_call(mods, singles, subblock):
    """both go through the same pass: the same status, counts and bytes, and the same parts and sub-parts on the chain"""
    torch, inf, _ = mods
    zr = importlib.import_module("zlib-ng_amd")
    for j in singles:
        rst, rn, rused, rparts, _, rwhole, rdst = _alone(torch, inf, zr, j, subblock)
        rsub = inf.inflate_large_last_subparts()
        rc, rows, rounds, launches, bufs = _run_batch(torch, inf, [j], subblock)
        st, n, used, msg, parts, subparts = rows[0]
        whole, dst = bufs[0]
        print(j.name, subblock, (rst, rn, rused, rparts, rsub), rows[0], rounds, launches)
        assert rc == 0 and rounds == 1, (j.name, rc, rounds)
        assert (st, n, used, msg) == (1, len(j.plain), len(j.comp), None) and (rst, rn, rused) == (st, n, used), (j.name, rows[0])
        assert torch.equal(dst[:n], rdst[:n]) and dst[:n].cpu().numpy().tobytes() == j.plain, j.name
        assert parts > 0 and (parts, subparts) == (rparts, rsub), (j.name, rows[0], rparts, rsub)
        assert launches == (2 if j.name == "runs-of-zeros" else 1), (j.name, launches)
        for w in (whole, rwhole):                         # nothing in front of the destination, nothing at or behind its end
            assert int(w[j.odd + j.cap:].min()) == 0xAB and int(w[:j.odd].min()) == 0xAB, j.name


def test_refusals_launch_nothing(mods, mixed):
    torch, inf, _ = mods
    jobs, _ = mixed
    stream = torch.cuda.Stream()
    some = jobs[:3]
    before = inf.workspace_bytes(stream)

    def refused(mutate=None, **kw):
        bufs = [j.dst(torch) for j in some]
        arr = inf.large_jobs([j.src for j in some], [b[1] for b in bufs], [j.window for j in some])
        for a in arr:
            a.status, a.out_len, a.in_used, a.parts, a.subparts = 77, 78, 79, 80, 81
        if mutate:
            mutate(arr)
        rc, rows, _, _ = inf.inflate_large_streams_dev([j.src for j in some], None, jobs=arr, stream=stream, **kw)
        assert rc == -3, (kw, rc)                         # ZNG_ROCM_EINVAL
        assert all(r[:3] == (77, 78, 79) and r[4:] == (80, 81) for r in rows), rows
        torch.cuda.synchronize()
        assert all(int(w.min()) == 0xAB for w, _ in bufs)
        assert inf.workspace_bytes(stream) == before

    def window_too_long(arr):
        arr[1].window_len = 32769
        arr[1].d_window = arr[1].d_src

    def null_src(arr):
        arr[2].d_src = None

    def null_window(arr):
        arr[0].d_window, arr[0].window_len = None, 100

    def null_dst(arr):
        arr[0].d_dst = None

    refused(flags=2)
    refused(flags=0x80000001)
    refused(round_bytes=4 * MiB - 1)
    refused(round_bytes=1)
    refused(round_bytes=2 << 30)
    refused(window_too_long)
    refused(null_src)
    refused(null_window)
    refused(null_dst)
    rc, rows, rounds, launches = inf.inflate_large_streams_dev([], [], stream=stream)
    assert (rc, rows, rounds, launches) == (0, [], 0, 0)
    assert inf.workspace_bytes(stream) == before


def test_two_host_threads_two_streams_two_batches(mods, mixed):
    """scratch is keyed by the caller's HIP stream and the counters are per thread: two host threads, each with a batch of
    its own on a stream of its own, several times over"""
    torch, inf, _ = mods
    jobs, refs = mixed
    halves = [jobs[0::2], jobs[1::2]]
    want = [[_dev(torch, j.plain) for j in h] for h in halves]
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            stream = torch.cuda.Stream()
            for rep in range(3):
                rc, rows, rounds, launches, bufs = _run_batch(torch, inf, halves[k], subblock=(k == 1), stream=stream)
                if rc != 0 or rounds != 1 or not 1 <= launches <= 2:
                    errors.append((k, rep, rc, rounds, launches))
                for j, row, (_, dst), w in zip(halves[k], rows, bufs, want[k]):
                    if row[:3] != (1, len(j.plain), len(j.comp)):
                        errors.append((k, rep, j.name, row))
                    elif not torch.equal(dst, w):
                        errors.append((k, rep, j.name, "bytes differ"))
        except Exception as e:                                               # noqa: BLE001 (reported below)
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
