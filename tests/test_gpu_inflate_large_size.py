"""The plaintext SIZE of large device-resident streams without decoding them (zng_rocm_uncompress_large_size_dev and
zng_rocm_uncompress_large_sizes_dev): a finder pass, ONE launch of the counting part kernel (inflate_large_size.hip) and the
chain walk, with a one-wavefront kernel on the device for every stream whose chain shows trouble.

Oracles, neither of them the code under test: the row zng_rocm_inflate_sizes_dev writes for the same bytes and history length
(one wavefront walks the whole stream; status, plaintext bytes, input consumed, message), and where a decode exists the
decode call (zng_rocm_inflate_large_dev, zng_rocm_uncompress_large_dev) and the plaintext's own length.  Shapes are the
smallest that reach the device path: it takes 128 KiB of input and four starts, so 2 .. 4 MiB of the synthetic mix."""
import importlib
import zlib

import numpy as np
import pytest

import synth
import wrapped_members as wm

pytestmark = pytest.mark.gpu

MiB = 1 << 20
TOO_FAR = "invalid distance too far back"


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), importlib.import_module("zlib-ng_amd.deflate"), zr


@pytest.fixture(scope="module")
def plain8():
    """the plaintext of test_gpu_inflate_large.py::test_history_in_front_of_the_stream"""
    return synth.silesia_like(8 << 20, seed=5).tobytes()


def _raw(plain, level, zdict=None, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy, zdict) if zdict else \
        zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(plain) + c.flush()


def _dev(torch, data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _small_rows(torch, inf, blobs, hist=0):
    """zng_rocm_inflate_sizes_dev's rows (status, out_len, in_used, message text) of raw streams, `hist` bytes of history"""
    offs, pos = [], 0
    for b in blobs:
        offs.append(pos)
        pos += (len(b) + 19) & ~3
    host = np.zeros(pos + 64, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        host[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    src = torch.from_numpy(host).cuda()
    b = inf.InflateDevBatch(src, offs, [len(x) for x in blobs], torch.empty(0, dtype=torch.uint8, device="cuda"),
                            [0] * len(blobs), [0] * len(blobs))
    for i in range(len(blobs)):
        b.jobs[i].out_ptr = None
        b.jobs[i].dict_len = hist
    b.run_sizes(0)
    return b.rows()


def _size(inf, zr, src, fmt=0, **kw):
    """the single call: (status, out_len, in_used, message text of a data error or "", parts)"""
    st, n, used, parts = inf.uncompress_large_size_dev(fmt, src, **kw)
    return st, n, used, zr.rocm.lib().zng_rocm_last_error().decode() if st == -3 else "", parts


def _agree(got, small):
    """the large call's answer against the small call's row: status, counts, and the text of a data error"""
    st, n, used, text = small
    assert got[:3] == (st, n, used), (got, small)
    if st == -3:
        assert got[3] == text, (got, small)
    if st != 1:
        assert got[4] == 0, got                          # no chain stands behind a stream that is not a valid one


@pytest.mark.parametrize("which", ["cpython1", "cpython6", "cpython9", "own6"])
def test_regular_streams_are_counted_on_their_chain(mods, which):
    torch, inf, dfl, zr = mods
    plain = synth.silesia_like(3 * MiB + 4321, seed=0x517E + len(which)).tobytes()
    if which == "own6":
        c, n = dfl.deflate_dev(_dev(torch, plain), level=6)
        comp = c[:n].cpu().numpy().tobytes()
    else:
        comp = _raw(plain, int(which[-1]))
    src = _dev(torch, comp)
    got = _size(inf, zr, src)
    assert got[:3] == (1, len(plain), len(comp))
    dst = torch.zeros(len(plain), dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(src, dst)
    assert (st, n, used) == (1, len(plain), len(comp)) and parts >= 4
    assert got[4] == parts, (got, parts, zr.rocm.lib().zng_rocm_last_error())
    _agree(got, _small_rows(torch, inf, [comp])[0])


def test_history_in_front_of_the_stream(mods, plain8):
    torch, inf, _, zr = mods
    zdict = plain8[-20000:]                               # the stream's first matches reach into the dictionary
    comp = _raw(plain8, 6, zdict)
    src = _dev(torch, comp)
    got = _size(inf, zr, src, dict_len=20000)             # (of the history only the length: no pointer)
    assert got[:3] == (1, len(plain8), len(comp)) and got[4] >= 4
    _agree(got, _small_rows(torch, inf, [comp], hist=20000)[0])
    assert _size(inf, zr, src, dict=_dev(torch, zdict)) == got
    none = _size(inf, zr, src)
    small = _small_rows(torch, inf, [comp])[0]
    assert small[0] == -3 and small[3] == TOO_FAR
    assert none[0] == -3 and none[3] == TOO_FAR and none[2] == small[2] and none[4] == 0
    _agree(none, small)
    # more history than the stream needs changes nothing; less is judged as the small call judges it
    assert _size(inf, zr, src, dict_len=32768)[:3] == got[:3]
    _agree(_size(inf, zr, src, dict_len=19999), _small_rows(torch, inf, [comp], hist=19999)[0])


def test_ratio_above_64_and_counts_above_32_bits(mods):
    torch, inf, _, zr = mods
    # a run: the decode path would run its part again with room for 1032 : 1; a counting part has no room to run out of
    comp = _raw(bytes(32 << 20), 6)
    src = _dev(torch, comp)
    rc, rows, rounds, launches = inf.uncompress_large_sizes_dev(0, [src])
    assert rc == 0 and rows[0][:4] == (1, 32 << 20, len(comp), None) and (rounds, launches) == (1, 1)
    _agree(_size(inf, zr, src), _small_rows(torch, inf, [comp])[0])
    # 70 x 64 MiB of zeros: 4.375 GiB of plaintext from about 4.5 MiB -- the count of the stream, and of nothing else, passes
    # 32 bits (the small call saturates at 0x7fffffff: the constructed length is the oracle)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    piece = c.compress(bytes(64 << 20)) + c.flush(zlib.Z_FULL_FLUSH)
    stream = piece * 70 + c.flush()
    assert 4 * MiB < len(stream) < 5 * MiB
    got = _size(inf, zr, _dev(torch, stream))
    assert got[:3] == (1, 70 * (64 << 20), len(stream)) and got[1] > 1 << 32
    assert got[4] >= 4, (got, zr.rocm.lib().zng_rocm_last_error())
    small = _small_rows(torch, inf, [stream])[0]
    assert small[:2] == (-5, 0x7fffffff)                  # (what the 64-bit count is for)


def test_irregular_streams_stay_on_the_device_with_the_decoders_verdict(mods, plain8):
    torch, inf, _, zr = mods
    plain = plain8[:2 * MiB]
    comp = _raw(plain, 6)
    flipped = bytearray(comp)
    flipped[len(comp) // 2] ^= 0x10
    text = b"About a hundred bytes of deflate data: a stream far too short for the finder to cut, sized by one wavefront, whole, now."
    tiny = _raw(text, 6)
    assert 90 <= len(tiny) <= 110                         # the 100-byte stream
    cases = {"truncated": comp[:len(comp) // 2], "flipped": bytes(flipped), "fixed": _raw(plain, 6, strategy=zlib.Z_FIXED),
             "tiny": tiny, "tiny-truncated": tiny[:50], "empty": b""}
    small = _small_rows(torch, inf, list(cases.values()))
    for (name, blob), row in zip(cases.items(), small):
        got = _size(inf, zr, _dev(torch, blob) if blob else None)
        _agree(got, row)
        if name in ("fixed", "tiny"):
            assert got[4] == 1, (name, got)              # what the finder does not cut is one part: the whole stream
    assert small[0][0] == -5 and small[2][:2] == (1, len(plain)) and small[3][:2] == (1, len(text))
    assert small[4][0] == -5 and small[5] == (-5, 0, 0, "input ended before the final block")


def test_single_byte_mutations_agree_with_the_small_call(mods, plain8):
    torch, inf, _, zr = mods
    plain = plain8[3 * MiB:5 * MiB]
    comp = _raw(plain, 6)
    clean = _size(inf, zr, _dev(torch, comp))
    assert clean[:3] == (1, len(plain), len(comp)) and clean[4] >= 4      # the chain, not the fallback alone
    rng = np.random.default_rng(0xB17F11B)
    n = len(comp)
    at = [int(v) for v in rng.integers(0, 64, 8)] + [int(v) for v in rng.integers(64, n - 64, 8)] + \
         [int(v) for v in rng.integers(n - 64, n, 8)]
    blobs = []
    for k, pos in enumerate(at):
        m = bytearray(comp)
        m[pos] ^= 1 << (k % 8)
        blobs.append(bytes(m))
    assert len(blobs) == 24
    small = _small_rows(torch, inf, blobs)
    srcs = [_dev(torch, b) for b in blobs]
    rc, rows, rounds, launches = inf.uncompress_large_sizes_dev(0, srcs)
    assert rc == 0 and launches == rounds
    for pos, row, want in zip(at, rows, small):
        _agree((row[0], row[1], row[2], row[3] or "", row[4]), want)
    assert any(w[0] != 1 for w in small)                  # (the mutations do damage streams)


def test_wrapped_members(mods, plain8):
    torch, inf, _, zr = mods
    plain = plain8[5 * MiB:7 * MiB + 77]
    dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    members = {1: zlib.compress(plain, 6), 2: wm.handmade(plain, 6, name=b"a name.bin", hcrc=True)}
    for fmt, member in members.items():
        src = wm.place(torch, member, 5)
        want = inf.uncompress_large_dev(fmt, src, dst)
        assert want[:3] == (1, len(plain), len(member))
        got = _size(inf, zr, src, fmt=fmt)
        assert got[:3] == want[:3] and got[4] >= 4
        # bytes behind the member are not consumed
        assert _size(inf, zr, wm.place(torch, member + b"behind", 3), fmt=fmt)[:3] == want[:3]
        # the input ends inside the trailer
        cut = _size(inf, zr, wm.place(torch, member[:-2], 7), fmt=fmt)
        assert cut[:3] == (-5, len(plain), len(member) - 2)
        assert inf.uncompress_large_dev(fmt, wm.place(torch, member[:-2], 7), dst)[:3] == cut[:3]
        # a bad header byte: the header's message
        bad = bytearray(member)
        bad[1] ^= 0x40
        rc, rows, _, _ = inf.uncompress_large_sizes_dev(fmt, [wm.place(torch, bytes(bad), 9)])
        assert rc == 0 and rows[0][:4] == (-3, 0, 0, "incorrect header check"), rows
        assert _size(inf, zr, wm.place(torch, bytes(bad), 9), fmt=fmt)[:4] == (-3, 0, 0, "incorrect header check")
    # a damaged check value: the decode says so, the sizing call -- which has no plaintext to check -- still answers 1
    bad = bytearray(members[2])
    bad[-6] ^= 0xff
    src = wm.place(torch, bytes(bad), 11)
    assert inf.uncompress_large_dev(2, src, dst)[0] == -3
    assert _size(inf, zr, src, fmt=2)[:3] == (1, len(plain), len(bad))
    # FDICT: the right dictionary, another one, none
    zdict = plain[-20000:]
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, zdict)
    member = c.compress(plain) + c.flush()
    src = wm.place(torch, member, 13)
    right, wrong = wm.place(torch, zdict, 1), wm.place(torch, zdict[:-1] + b"\x00\x01", 3)
    rc, rows, _, _ = inf.uncompress_large_sizes_dev(1, [src, src, src], dicts=[right, wrong, None])
    assert rc == 0
    assert rows[0][:4] == (1, len(plain), len(member), None) and rows[0][4] >= 4
    assert rows[1][:4] == (-3, 0, 0, None) and rows[2][:4] == (2, 0, 6, None)
    want = inf.uncompress_large_streams_dev(1, [src, src, src], [dst, dst, dst], dicts=[right, wrong, None])[1]
    assert [r[:4] for r in rows] == [r[:4] for r in want]
    assert _size(inf, zr, src, fmt=1, dict=right)[:3] == rows[0][:3]
    assert _size(inf, zr, src, fmt=1)[:3] == (2, 0, 6)


def test_batch_equals_the_single_calls_in_one_launch_per_round(mods, plain8):
    torch, inf, _, zr = mods
    regular = [_raw(synth.silesia_like(mib * MiB + 11 * mib, seed=0xBA7C + mib).tobytes(), 6) for mib in (1, 2, 4)]
    whole = _raw(plain8[:4 * MiB], 6)
    blobs = regular + [_raw(plain8[:2 * MiB], 6, strategy=zlib.Z_FIXED), whole[:len(whole) // 2], _raw(b"tiny " * 20, 6)]
    srcs = [_dev(torch, b) for b in blobs]
    alone = [_size(inf, zr, s) for s in srcs]
    assert [a[0] for a in alone] == [1, 1, 1, 1, -5, 1] and all(a[4] >= 4 for a in alone[:3])
    sentinel = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")

    def rounds_by_rule(round_bytes):
        n, run = 0, None
        for b in blobs:
            if run is None or run + len(b) > round_bytes:
                n, run = n + 1, 0
            run += len(b)
        return n

    for round_bytes in (0, 4 * MiB):
        jobs = inf.large_jobs(srcs, [sentinel] * len(srcs))
        rc, rows, rounds, launches = inf.uncompress_large_sizes_dev(0, srcs, round_bytes=round_bytes, jobs=jobs)
        assert rc == 0
        for row, a in zip(rows, alone):
            assert (row[0], row[1], row[2], row[3] or "", row[4]) == a and row[5] == 0, (row, a)
        assert launches == rounds == rounds_by_rule(round_bytes or 256 * MiB), (rounds, launches)
        assert int(sentinel.min()) == 0xA5 and int(sentinel.max()) == 0xA5
    assert rounds_by_rule(4 * MiB) >= 2                   # (the shapes do split into rounds)
    # flags: none are taken, and nothing is written
    jobs = inf.large_jobs(srcs, [sentinel] * len(srcs))
    rc, rows, _, _ = inf.uncompress_large_sizes_dev(0, srcs, flags=inf.SUBBLOCK, jobs=jobs)
    assert rc == -3 and "0x1" in zr.rocm.lib().zng_rocm_last_error().decode() and all(r[:3] == (0, 0, 0) for r in rows)


def test_scratch_stays_far_below_the_decodes(mods, plain8):
    torch, inf, _, zr = mods
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    piece = c.compress(plain8) + c.flush(zlib.Z_FULL_FLUSH)
    stream = piece * 5 + c.flush()                        # five independent copies: 40 MiB of plaintext
    assert len(stream) >= 16 * MiB
    src = _dev(torch, stream)
    s = torch.cuda.Stream()
    before = inf.workspace_bytes(s)
    st, n, used, parts = inf.uncompress_large_size_dev(0, src, stream=s)
    grown = inf.workspace_bytes(s) - before
    print("sizing %d compressed bytes in %d parts: workspace grew by %d bytes (%.3f per compressed byte)"
          % (len(stream), parts, grown, grown / len(stream)))
    assert (st, n, used) == (1, 5 * len(plain8), len(stream)) and parts >= 4
    # the decode reserves 128 bytes of part slots per compressed byte alone; the counting pass the finder's candidate tables
    # and under 100 bytes per part
    assert 0 < grown < len(stream)
    zr.rocm.lib().zng_rocm_stream_release(s.cuda_stream)
