"""Parts that begin INSIDE a block (zng_rocm_inflate_large_ex_dev with ZNG_ROCM_INFLATE_SUBBLOCK): a stream of fixed-Huffman
blocks, which offers no block start to find, and the long blocks of a foreign stream are cut at symbol boundaries that a
dry parse finds on the device.  The loop replaced is inflate_fast (inffast_tpl.h:151-298) with the headers around it
(inflate.c:735-917).  Oracle: the plaintext, CPython's zlib for the streams, the sequential decoder for damaged ones."""
import importlib
import threading
import zlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), importlib.import_module("zlib-ng_amd.deflate"), zr


def _raw(plain, level, strategy=zlib.Z_DEFAULT_STRATEGY, zdict=None):
    if zdict is not None:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy, zdict)
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(plain) + c.flush()


def zr_error():
    return importlib.import_module("zlib-ng_amd").rocm.lib().zng_rocm_last_error().decode()


def _dev(torch, data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _check_exact(torch, inf, comp, plain, min_parts=64, min_sub=32):
    src = _dev(torch, comp)
    dst = torch.zeros(len(plain) + 4096, dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(src, dst, subblock=True)
    subparts = inf.inflate_large_last_subparts()
    assert (st, n, used) == (1, len(plain), len(comp)), (st, n, used, parts)
    assert parts >= min_parts and subparts >= min_sub, (parts, subparts, zr_error())
    assert dst[:n].cpu().numpy().tobytes() == plain
    assert int(dst[n:].max()) == 0                        # nothing written behind the end
    return parts, subparts


def test_cpython_fixed_stream_is_cut_inside_its_blocks(mods):
    torch, inf, _, _ = mods
    plain = synth.silesia_like(32 << 20, seed=0xF1ED).tobytes()
    comp = _raw(plain, 6, zlib.Z_FIXED)
    _check_exact(torch, inf, comp, plain)
    # flags 0: nothing to cut at, the sequential decoder (as zng_rocm_inflate_large_dev)
    dst = torch.zeros(len(plain), dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(_dev(torch, comp), dst)
    assert (st, n, used, parts) == (1, len(plain), len(comp), 0)
    assert inf.inflate_large_last_subparts() == 0


def test_sub_starts_are_landed_on(mods):
    """nearly every sub-start the dry parse placed in a fixed-code stream is a true symbol boundary (99.9 % on the CPU,
    tests/test_subblock_sync_cpu.py), and the genuine decode passes all of them: nearly all must become parts on the chain"""
    torch, inf, _, _ = mods
    plain = synth.silesia_like(32 << 20, seed=0x1A4D).tobytes()
    comp = _raw(plain, 6, zlib.Z_FIXED)
    _, subparts = _check_exact(torch, inf, comp, plain)
    placed = inf.inflate_large_last_substarts()
    assert placed > 0 and subparts >= 0.95 * placed, (subparts, placed)


def test_own_quick_stream_one_final_static_block(mods):
    """deflate_quick_dev writes ONE final fixed-code block per job, with no marker in it: every part but the first begins
    inside that block, and the chain ends at the first end of block behind the final block's sub-starts"""
    torch, inf, dfl, _ = mods
    plain = synth.silesia_like(32 << 20, seed=0x0C1C, seg_bytes=1 << 20)
    q = dfl.QuickBatch(torch.from_numpy(plain).cuda(), [0], [plain.size])
    q.run()
    torch.cuda.synchronize()
    comp = q.compressed(0)
    d = zlib.decompressobj(-15)
    assert d.decompress(comp) == plain.tobytes() and d.eof
    _check_exact(torch, inf, comp, plain.tobytes())


@pytest.mark.parametrize("level", [6, 9])
def test_cpython_dynamic_blocks_are_split(mods, level):
    import inflate_util
    torch, inf, _, _ = mods
    plain = synth.silesia_like(32 << 20, seed=0xD1A0 + level).tobytes()
    comp = _raw(plain, level)
    status, blocks = inflate_util.oracle_block_starts(comp, len(plain))
    assert status == 1
    parts, _ = _check_exact(torch, inf, comp, plain, min_parts=len(blocks) + 64)


def test_own_level6_stream_keeps_its_parts(mods):
    torch, inf, dfl, _ = mods
    plain = synth.silesia_like(32 << 20, seed=78)
    src_plain = torch.from_numpy(plain).cuda()
    comp, clen = dfl.deflate_dev(src_plain, level=6)
    src = comp[:clen].contiguous()
    dst = torch.zeros(plain.size, dtype=torch.uint8, device="cuda")
    st0, n0, used0, parts0 = inf.inflate_large_dev(src, dst)
    assert (st0, n0, used0) == (1, plain.size, clen) and parts0 >= 8
    dst.zero_()
    st, n, used, parts = inf.inflate_large_dev(src, dst, subblock=True)
    assert (st, n, used) == (1, plain.size, clen) and parts >= parts0
    assert torch.equal(dst, src_plain)


def test_bytes_behind_a_fixed_stream(mods):
    """the final block is a fixed-code one that sub-parts begin inside: in_used is where it ends, not the input's end"""
    torch, inf, _, _ = mods
    plain = synth.silesia_like(8 << 20, seed=0xBE1D).tobytes()
    comp = _raw(plain, 6, zlib.Z_FIXED)
    tail = np.random.default_rng(8).integers(0, 256, size=8, dtype=np.uint8).tobytes()
    src = _dev(torch, comp + tail)
    dst = torch.zeros(len(plain) + 4096, dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(src, dst, subblock=True)
    assert (st, n, used) == (1, len(plain), len(comp)), (st, n, used, parts)
    assert parts >= 8 and inf.inflate_large_last_subparts() >= 4
    assert dst[:n].cpu().numpy().tobytes() == plain


def test_dictionary_in_front_of_a_fixed_stream(mods):
    torch, inf, _, _ = mods
    plain = synth.silesia_like(8 << 20, seed=0xD1C7).tobytes()
    zdict = plain[-20000:]
    comp = _raw(plain, 6, zlib.Z_FIXED, zdict)
    src = _dev(torch, comp)
    win = _dev(torch, zdict)
    dst = torch.zeros(len(plain), dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(src, dst, window=win, subblock=True)
    assert (st, n, used) == (1, len(plain), len(comp)) and parts >= 8
    assert dst.cpu().numpy().tobytes() == plain
    st2, _, _, parts2 = inf.inflate_large_dev(src, dst, subblock=True)
    assert st2 == -3 and parts2 == 0                      # too far back without it: the sequential decoder's answer


def test_mixed_fixed_then_dynamic_stream(mods):
    torch, inf, _, _ = mods
    a = synth.silesia_like(6 << 20, seed=0x313).tobytes()
    b = synth.silesia_like(6 << 20, seed=0x314).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    comp = c.compress(a) + c.flush(zlib.Z_SYNC_FLUSH) + _raw(b, 6)
    _check_exact(torch, inf, comp, a + b, min_parts=16, min_sub=8)


@pytest.mark.parametrize("kind", ["fixed", "level9"])
def test_mutated_streams_agree_with_the_sequential_decoder(mods, kind):
    """20 mutations each (bit flips, byte edits, a zeroed run, truncations) inside a 4 MiB stream: status, bytes produced,
    bytes used and the bytes before an error as the sequential decoder gives them"""
    torch, inf, _, zr = mods
    rng = np.random.default_rng(0x5B + (kind == "fixed"))
    plain = synth.silesia_like(4 << 20, seed=43, seg_bytes=256 << 10).tobytes()
    comp = _raw(plain, 6, zlib.Z_FIXED) if kind == "fixed" else _raw(plain, 9)
    dst = torch.zeros(len(plain) + 4096, dtype=torch.uint8, device="cuda")
    # the clean stream is cut inside its blocks: the mutations below go through the SUBBLOCK path, not around it
    st, n, used, parts = inf.inflate_large_dev(_dev(torch, comp), dst, subblock=True)
    assert (st, n, used) == (1, len(plain), len(comp)) and parts > 0 and inf.inflate_large_last_subparts() > 0, \
        (parts, inf.inflate_large_last_subparts(), zr_error())
    for k in range(20):
        bad = bytearray(comp)
        m = k % 4
        at = int(rng.integers(64, len(bad) - 64))
        if m == 0:
            bad[at] ^= 1 << int(rng.integers(0, 8))
        elif m == 1:
            bad[at] = int(rng.integers(0, 256))
            bad[at + 1] = int(rng.integers(0, 256))
        elif m == 2:
            bad[at:at + 16] = bytes(16)
        else:
            bad = bad[:at]
        bad = bytes(bad)
        ref = inf.decode_tokens(bad)
        dst.zero_()
        st, n, used, _ = inf.inflate_large_dev(_dev(torch, bad), dst, subblock=True)
        assert (st, n) == (ref.status, ref.out_len), (kind, k, m, at, st, n, ref.status, ref.out_len)
        if ref.status == 1:
            assert used == ref.in_used, (kind, k, m, at)
        if n:
            assert torch.equal(dst[:n], inf.resolve_dev(ref)[:n]), (kind, k, m, at)


def test_small_streams_and_unknown_flags(mods):
    import ctypes as C
    torch, inf, _, zr = mods
    plain = synth.silesia_like(200 << 10, seed=12).tobytes()
    comp = _raw(plain, 6, zlib.Z_FIXED)
    assert len(comp) < (128 << 10)
    src = _dev(torch, comp)
    dst = torch.zeros(len(plain), dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(src, dst, subblock=True)
    assert (st, n, used, parts) == (1, len(plain), len(comp), 0)
    assert inf.inflate_large_last_subparts() == 0
    assert dst.cpu().numpy().tobytes() == plain
    lib = zr.rocm.lib()
    dst.fill_(0x5A)
    torch.cuda.synchronize()
    out_len, in_used = C.c_uint64(77), C.c_size_t(77)
    for flags in (2, 0x80000000, 3):
        rc = lib.zng_rocm_inflate_large_ex_dev(zr.rocm._dev_ptr(src), len(comp), None, 0, zr.rocm._dev_ptr(dst),
                                               int(dst.numel()), C.byref(out_len), C.byref(in_used), flags, None)
        assert rc == -3 and (out_len.value, in_used.value) == (0, 0), flags
        assert "flag" in lib.zng_rocm_last_error().decode()
    torch.cuda.synchronize()
    assert int(dst.min()) == 0x5A and int(dst.max()) == 0x5A


def test_two_host_threads_keep_their_own_counters(mods):
    torch, inf, _, _ = mods
    plains = [synth.silesia_like(12 << 20, seed=900 + k).tobytes() for k in range(2)]
    comps = [_raw(p, 6, zlib.Z_FIXED) for p in plains]
    srcs = [_dev(torch, c) for c in comps]
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            stream = torch.cuda.Stream()
            dst = torch.zeros(len(plains[k]) + 64, dtype=torch.uint8, device="cuda")
            for rep in range(3):
                dst.zero_()
                torch.cuda.current_stream().synchronize()
                st, n, used, parts = inf.inflate_large_dev(srcs[k], dst, stream=stream, subblock=(rep != 1))
                sub = inf.inflate_large_last_subparts()
                if rep == 1:
                    if (st, n, used, parts, sub) != (1, len(plains[k]), len(comps[k]), 0, 0):
                        errors.append((k, rep, st, n, used, parts, sub))
                elif (st, n, used) != (1, len(plains[k]), len(comps[k])) or parts < 16 or sub < 8 or sub >= parts:
                    errors.append((k, rep, st, n, used, parts, sub))
                if dst[:n].cpu().numpy().tobytes() != plains[k]:
                    errors.append((k, rep, "bytes differ"))
        except Exception as e:                                               # noqa: BLE001 (reported below)
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
