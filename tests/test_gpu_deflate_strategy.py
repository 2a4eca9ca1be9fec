"""GPU: zlib's strategies on the device -- Z_HUFFMAN_ONLY and Z_RLE through their own front end (deflate_rle.h), Z_FIXED
through the forced-static block emitter -- via zng_rocm_deflate_strategy_block_dev / _strategy_streams_dev and the hook's
zng_rocm_hook_deflate_block_strategy.  Every output is read back by CPython's zlib and by the product's inflater."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import inflate_util
import strategy_util as su
import synth
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu

STRATEGIES = (su.Z_DEFAULT_STRATEGY, su.Z_FILTERED, su.Z_HUFFMAN_ONLY, su.Z_RLE, su.Z_FIXED)


@pytest.fixture(scope="module")
def mods():
    zr = product()
    zr.init()
    return zr, importlib.import_module("zlib-ng_amd.deflate"), importlib.import_module("zlib-ng_amd.inflate")


def _dev(data, front=b""):
    torch = torch_mod()
    return torch.from_numpy(np.frombuffer(front + data + b"\0" * 16, dtype=np.uint8).copy()).cuda()


def _deflate(dfl, data, level, strategy, dict_bytes=b"", flags=0):
    src = _dev(data, dict_bytes)
    dst, clen = dfl.deflate_dev(src, level=level, length=len(data), offset=len(dict_bytes), dict_len=len(dict_bytes),
                                flags=flags, strategy=strategy)
    assert clen <= dfl.deflate_bound(len(data))
    return dst[:clen].cpu().numpy().tobytes()


def _check_round_trip(inf, comp, data):
    d = zlib.decompressobj(-15)
    assert d.decompress(comp) == data and d.eof and d.unused_data == b""
    dec = inf.decode_tokens(comp)
    assert dec.status == 1
    assert inf.resolve_dev(dec).cpu().numpy().tobytes() == data


def _cases():
    rng = np.random.default_rng(5)
    return {
        "empty": b"",
        "one": b"z",
        "two": b"zz",
        "zeros3MiB": bytes(3 << 20),
        "random": rng.integers(0, 256, size=(1 << 20) + 333, dtype=np.uint8).tobytes(),
        "runs": su.run_heavy((2 << 20) + 77, seed=8),
    }


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("level", [1, 6, 9])
def test_round_trip(mods, strategy, level):
    zr, dfl, inf = mods
    for name, data in _cases().items():
        comp = _deflate(dfl, data, level, strategy)
        _check_round_trip(inf, comp, data)
        st, msg, out, used = inflate_util.oracle_inflate(comp, cap=len(data) + 16)
        assert st == 1 and out == data and used == len(comp), (name, st, msg)


def test_round_trip_silesia_like(mods):
    zr, dfl, inf = mods
    data = synth.silesia_like(16 << 20, seed=31).tobytes()
    for strategy in STRATEGIES:
        _check_round_trip(inf, _deflate(dfl, data, 6, strategy), data)


def test_rle_parity_single_segment(mods):
    """token for token the parse of deflate_rle.c (strategy_util.rle_parse), with and without history in front"""
    zr, dfl, inf = mods
    rng = np.random.default_rng(17)
    for s in range(8):
        data = su.run_heavy(int(rng.integers(1000, 120000)), seed=200 + s)
        hist = su.run_heavy(int(rng.integers(1, 32768)), seed=300 + s) if s % 2 else b""
        if s % 4 == 3:                                       # the block continues the history's last run
            hist += data[:1] * 5
        comp = _deflate(dfl, data, 6, su.Z_RLE, dict_bytes=hist)
        want = su.rle_parse(hist + data, start=len(hist))
        assert su.tokens_of(comp, window_len=len(hist)) == want, s
        assert zlib.decompressobj(-15, zdict=hist).decompress(comp) == data if hist else True


def test_rle_large_inputs_match_at_distance_one(mods):
    zr, dfl, inf = mods
    for data in (su.run_heavy(5 << 20, seed=4), bytes(3 << 20), synth.silesia_like(4 << 20, seed=2).tobytes()):
        comp = _deflate(dfl, data, 6, su.Z_RLE)
        _check_round_trip(inf, comp, data)
        dec = inf.decode_tokens(comp)
        m = dec.tokens[(dec.tokens & 0x80000000) != 0]
        assert m.size and np.all((m & 0xffff) == 0)          # distance 1


def test_huffman_only_has_no_match(mods):
    zr, dfl, inf = mods
    for data in (bytes(3 << 20), su.run_heavy(1 << 20, seed=6), synth.silesia_like(2 << 20, seed=3).tobytes()):
        for level in (1, 9):
            comp = _deflate(dfl, data, level, su.Z_HUFFMAN_ONLY)
            _check_round_trip(inf, comp, data)
            dec = inf.decode_tokens(comp)
            assert not np.any(dec.tokens & 0x80000000)


def test_fixed_never_writes_a_dynamic_block(mods):
    zr, dfl, inf = mods
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, size=(1 << 20) + 5, dtype=np.uint8).tobytes()
    for data in (synth.silesia_like(3 << 20, seed=8).tobytes(), noise, b"the quick brown fox " * 5000):
        comp = _deflate(dfl, data, 6, su.Z_FIXED)
        _check_round_trip(inf, comp, data)
        st, blocks = inflate_util.oracle_block_starts(comp, len(data) + 16)
        assert st == 1 and blocks
        assert all(bt != 2 for _, bt in blocks)
        if data is not noise:
            assert any(bt == 1 for _, bt in blocks)
    # incompressible input: stored, within zng_rocm_deflate_bound
    comp = _deflate(dfl, noise, 6, su.Z_FIXED)
    assert len(comp) <= dfl.deflate_bound(len(noise))


def test_size_against_cpython_same_strategy(mods):
    """within 3 % of CPython's size with the same strategy -- except Z_FIXED, bound at 8 %: the level's matcher prices
    its shortest-path parse with the segment's own (dynamic-code) symbol costs, not the static code's, and a static-code
    cost model for that parse is not part of this path (measured on this input: 1.060 x CPython)"""
    zr, dfl, inf = mods
    data = synth.silesia_like(16 << 20, seed=12).tobytes()
    for strategy in STRATEGIES:
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
        ref = len(c.compress(data) + c.flush())
        got = len(_deflate(dfl, data, 6, strategy))
        assert got <= (1.08 if strategy == su.Z_FIXED else 1.03) * ref, (strategy, got, ref)


def test_default_and_filtered_are_unchanged(mods):
    zr, dfl, inf = mods
    torch = torch_mod()
    lib = zr.rocm.lib()
    data = synth.silesia_like(3 << 20, seed=14).tobytes()
    src = _dev(data)
    for level in (0, 1, 6, 9):
        base, blen = dfl.deflate_dev(src, level=level, length=len(data))
        base = base[:blen].cpu().numpy().tobytes()
        for strategy in (su.Z_DEFAULT_STRATEGY, su.Z_FILTERED):
            cap = dfl.deflate_bound(len(data))
            dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
            out_len = C.c_size_t(0)
            rc = lib.zng_rocm_deflate_strategy_block_dev(level, strategy, src.data_ptr(), len(data), 0, 0, dst.data_ptr(),
                                                         cap, C.byref(out_len), None)
            assert rc == 0
            assert dst[:out_len.value].cpu().numpy().tobytes() == base, (level, strategy)
    # many streams
    sizes = [0, 1, 70000, 300000, 1 << 20]
    offs = np.cumsum([0] + sizes[:-1]).tolist()
    buf = synth.silesia_like(sum(sizes), seed=15).tobytes()
    src = _dev(buf)
    b0 = dfl.StreamsBatch(src, offs, sizes)
    b0.run(level=6)
    want = [b0.compressed(i) for i in range(len(sizes))]
    for strategy in (su.Z_DEFAULT_STRATEGY, su.Z_FILTERED):
        b1 = dfl.StreamsBatch(src, offs, sizes)
        rc = lib.zng_rocm_deflate_strategy_streams_dev(6, strategy, C.byref(b1.jobs), b1.n, C.byref(b1.out_lens), None)
        assert rc == 0
        assert [b1.compressed(i) for i in range(len(sizes))] == want


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_many_streams(mods, strategy):
    zr, dfl, inf = mods
    rng = np.random.default_rng(40 + strategy)
    sizes = [int(v) for v in rng.choice([0, 1, 2, 100, 5000, 70000, 200000], size=256)]
    offs = np.cumsum([0] + sizes[:-1]).tolist()
    buf = (su.run_heavy(sum(sizes) // 2 + 1, seed=strategy) +
           synth.silesia_like(sum(sizes) // 2 + 1, seed=strategy).tobytes())[:sum(sizes)]
    batch = dfl.StreamsBatch(_dev(buf), offs, sizes)
    lens = batch.run(level=6, strategy=strategy)
    assert len(lens) == 256
    for i in range(256):
        comp = batch.compressed(i)
        d = zlib.decompressobj(-15)
        assert d.decompress(comp) == buf[offs[i]:offs[i] + sizes[i]] and d.eof, i


def test_strategy_out_of_range_is_refused(mods):
    zr, dfl, inf = mods
    torch = torch_mod()
    lib = zr.rocm.lib()
    data = b"abc" * 1000
    src = _dev(data)
    cap = dfl.deflate_bound(len(data))
    dst = torch.full((cap,), 0x5a, dtype=torch.uint8, device="cuda")
    out_len = C.c_size_t(123)
    for strategy in (-1, 5, 99):
        rc = lib.zng_rocm_deflate_strategy_block_dev(6, strategy, src.data_ptr(), len(data), 0, 0, dst.data_ptr(), cap,
                                                     C.byref(out_len), None)
        assert rc == -3                                          # ZNG_ROCM_EINVAL
        b = dfl.StreamsBatch(src, [0], [len(data)])
        assert lib.zng_rocm_deflate_strategy_streams_dev(6, strategy, C.byref(b.jobs), 1, C.byref(b.out_lens), None) < 0
    torch.cuda.synchronize()
    assert out_len.value == 123
    assert bool((dst == 0x5a).all())
    with pytest.raises(Exception):
        dfl.deflate_dev(src, level=6, length=len(data), strategy=5)


class _Hook:
    def __init__(self, lib):
        self.lib = lib
        self.h = C.c_void_p()
        assert lib.zng_rocm_hook_create(C.byref(self.h), 1 << 20) == 0

    def block(self, data, level, strategy, flags, check, cv):
        data = bytes(data)
        buf = C.create_string_buffer(data, max(len(data), 1))
        cap = self.lib.zng_rocm_hook_deflate_bound(len(data))
        out = C.create_string_buffer(cap)
        v, n = C.c_uint32(cv), C.c_size_t(0)
        rc = self.lib.zng_rocm_hook_deflate_block_strategy(self.h, level, strategy, C.addressof(buf), len(data), flags, check,
                                                           C.byref(v), C.addressof(out), cap, C.byref(n))
        return rc, out.raw[:n.value], int(v.value)

    def close(self):
        self.lib.zng_rocm_hook_destroy(self.h)


def test_hook_block_sequences_switch_strategy(mods):
    """dict_len history + ZNG_ROCM_BLOCK_NOT_FINAL blocks through the strategy hook, the strategy changing from block to
    block: the concatenation is one stream, Adler-32 and CRC-32 continue across the blocks"""
    zr, dfl, inf = mods
    lib = zr.rocm.lib()
    data = su.run_heavy(3 << 20, seed=51) + synth.silesia_like(3 << 20, seed=52).tobytes()
    cuts = [0, 700000, 700001, 2 << 20, 3500000, 5000000, len(data)]
    order = [su.Z_RLE, su.Z_HUFFMAN_ONLY, su.Z_FIXED, su.Z_DEFAULT_STRATEGY, su.Z_RLE, su.Z_FILTERED]
    for check in (1, 2):
        h = _Hook(lib)
        try:
            cv = 1 if check == 1 else 0
            comp = b""
            for k in range(len(cuts) - 1):
                last = k == len(cuts) - 2
                rc, blk, cv = h.block(data[cuts[k]:cuts[k + 1]], 6 if k % 2 else 1, order[k], 0 if last else dfl.BLOCK_NOT_FINAL,
                                      check, cv)
                assert rc == 0, k
                comp += blk
            assert h.block(b"x", 6, 5, 0, check, cv)[0] != 0          # refused, nothing changes
        finally:
            h.close()
        d = zlib.decompressobj(-15)
        assert d.decompress(comp) == data and d.eof
        assert cv == (zlib.adler32(data) if check == 1 else zlib.crc32(data))
