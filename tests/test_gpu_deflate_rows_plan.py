"""GPU: the border shapes of tests/test_deflate_rows_plan_cpu.py through the device, so that the table the kernels receive is
the one that test describes (deflate_rows_plan.h: streams into segments of 128 KiB, segments into blocks at every 61440 positions
counted from the 1024-byte batch that holds the segment's first position, positions counted from the first history byte).

  streams   in_len {0, 1, 1024, 61441, 131072, 131073} x dict_len {0, 1000, 32768}, low-entropy text so that matches cross the
            borders and reach into the history: one zng_rocm_deflate_window_streams_dev call at level 1 and one at level 6
  one       the longest length, with each history, through zng_rocm_deflate_block_dev and zng_rocm_deflate_async_dev; the block
            call, the async call and the streams call over that single stream give the same bytes
  bound     zng_rocm_deflate_bound is the rule of the plan
Every output is inflated by CPython's zlib.decompressobj(-15, zdict = the history) and compared with the plaintext."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import matcher_cases as mc
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu

IN_LENS = (0, 1, 1024, 61441, 131072, 131073)
DICT_LENS = (0, 1000, 32768)
WORDS = (b"segment ", b"block ", b"border ", b"batch ", b"history ", b"window ", b"the ", b"of ", b"61440 ", b"1024 ", b"\n")


def _text(n, seed):
    rng = np.random.default_rng(seed)
    out = b"".join(WORDS[i] for i in rng.integers(0, len(WORDS), size=n // 4 + 8))
    assert len(out) >= n
    return out[:n]


def _inflate(comp, history):
    d = zlib.decompressobj(-15, zdict=history) if history else zlib.decompressobj(-15)
    data = d.decompress(comp) + d.flush()
    return data, d.eof, d.unused_data


@pytest.fixture(scope="module")
def dev():
    zr = product()
    zr.init()

    class Dev:
        torch = torch_mod()
        dfl = importlib.import_module("zlib-ng_amd.deflate")
        rocm = importlib.import_module("zlib-ng_amd.rocm")
    Dev.lib = Dev.rocm.lib()
    return Dev


@pytest.fixture(scope="module")
def streams(dev):
    """[(history, plaintext)] and their packed copy on the device"""
    whole = _text(32768 + max(IN_LENS), 0xB10C)
    items = [(whole[32768 - d:32768], whole[32768:32768 + n]) for n in IN_LENS for d in DICT_LENS]
    assert sum(len(h) + len(p) for h, p in items) < 3 << 20
    host, offs, lens, dls = mc.pack(items)
    return items, dev.torch.from_numpy(host).cuda(), offs, lens, dls


def _streams_call(dev, src, offs, lens, dls, level):
    b = dev.dfl.StreamsBatch(src, offs, lens, dict_len=dls)
    b.dst.zero_()
    rc = dev.lib.zng_rocm_deflate_window_streams_dev(level, 0, 15, C.byref(b.jobs), b.n, C.byref(b.out_lens), dev.rocm._stream_ptr(None))
    dev.torch.cuda.synchronize()
    assert rc == 0, rc
    return [b.compressed(i) for i in range(b.n)]


@pytest.mark.parametrize("level", (1, 6))
def test_border_shapes_as_one_batch(dev, streams, level):
    items, src, offs, lens, dls = streams
    comps = _streams_call(dev, src, offs, lens, dls, level)
    for (history, plain), comp in zip(items, comps):
        assert _inflate(comp, history) == (plain, True, b""), (level, len(plain), len(history))
        assert len(comp) <= dev.dfl.deflate_bound(len(plain))


@pytest.mark.parametrize("level", (1, 6))
def test_one_stream_calls_give_the_bytes_of_the_streams_call(dev, streams, level):
    torch = dev.torch
    items, src, offs, lens, dls = streams
    n = max(IN_LENS)
    for i in (k for k in range(len(items)) if lens[k] == n):
        history, plain = items[i]
        alone = _streams_call(dev, src, offs[i:i + 1], lens[i:i + 1], dls[i:i + 1], level)[0]
        dst, got = dev.dfl.deflate_dev(src, level=level, length=n, offset=offs[i], dict_len=dls[i])
        block = dst[:got].cpu().numpy().tobytes()
        adst = torch.zeros(dev.dfl.deflate_bound(n), dtype=torch.uint8, device="cuda")
        res = torch.zeros(2, dtype=torch.int64, device="cuda")
        dev.dfl.deflate_async_dev(src, adst, res, level=level, length=n, offset=offs[i], dict_len=dls[i])
        torch.cuda.synchronize()
        size, too_long = res.cpu().tolist()
        assert too_long == 0
        assert _inflate(block, history) == (plain, True, b""), (level, dls[i])
        assert block == alone and adst[:size].cpu().numpy().tobytes() == block, (level, dls[i])


def test_bound_is_the_plans(dev):
    for n in (0, 1, 131072, 131073, 262144, 262145, (1 << 32) - 1, 1 << 32):
        assert dev.dfl.deflate_bound(n) == n + n // 8 + (-(-n // 131072) if n else 1) * 1032 + 16, n
