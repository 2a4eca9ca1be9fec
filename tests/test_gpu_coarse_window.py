"""GPU: the coarse adapter (integration/arch/rocm/rocm_deflate.c) for streams opened with a window below 32 KiB
(deflateInit2's windowBits; s->w_bits 9 and 12), raw, zlib and gzip, through a driver of its own (tests/c/coarse_window_driver.c:
the existing drivers fix w_bits = 15).  CPython's zlib is the reader that really has a 1 << w window: decompressobj at that
window, fed 97 output bytes at a time so that copies go through its window, which also verifies the trailer the adapter's check
value went into."""
import importlib
import os
import subprocess
import zlib

import numpy as np
import pytest

import strategy_util as su
import synth
import window_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """strict C11, the flags of test_abi_c11.py"""
    zr = importlib.import_module("zlib-ng_amd")
    libdir = os.path.dirname(zr.lib_path())
    exe = str(tmp_path_factory.mktemp("coarse_window") / "coarse_window_driver")
    arch = os.path.join(ROOT, "integration", "arch", "rocm")
    cmd = ["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-DZNG_ROCM_STANDALONE_CHECK",
           "-DROCM_MIN_BYTES=1024", "-DROCM_INFLATE_MIN_BYTES=1", "-DROCM_DEFLATE_BLOCK_BYTES=1048576",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "c"), "-I" + arch,
           os.path.join(ROOT, "tests", "c", "coarse_window_driver.c")] + \
          [os.path.join(arch, f) for f in ("rocm_deflate.c", "rocm_inflate.c", "rocm_slots.c", "rocm_features.c")] + \
          ["-o", exe, "-L" + libdir, "-lzng_rocm", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    return exe


def run_driver(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    return p.stdout.strip()


def test_driver_compiles_as_strict_c11_and_falls_back_without_a_gpu(driver, tmp_path):
    """no GPU needed: without a device the adapter declines and the driver says so (with one, the tests below say more)"""
    zr = importlib.import_module("zlib-ng_amd")
    if zr.device_count() > 0:
        return
    (tmp_path / "in.bin").write_bytes(synth.silesia_like(1 << 18, seed=7).tobytes())
    assert run_driver(driver, "d", 6, 1, 9, 1 << 16, 0, tmp_path / "in.bin", tmp_path / "out.z") == "fallback"
    assert run_driver(driver, "g", 9, 512, tmp_path / "in.bin", tmp_path / "out.z") == "fallback"


@pytest.mark.gpu
@pytest.mark.parametrize("wrap", [0, 1, 2])
@pytest.mark.parametrize("w", [9, 12])
def test_adapter_at_a_small_window(driver, tmp_path, w, wrap):
    plain = su.run_heavy(3 << 19, seed=70 + wrap) + synth.silesia_like(3 << 19, seed=71 + wrap).tobytes()
    assert len(plain) == 3 << 20
    (tmp_path / "in.bin").write_bytes(plain)
    line = run_driver(driver, "d", 6, wrap, w, 700001, 0, tmp_path / "in.bin", tmp_path / "out.z")
    assert line.startswith("device %d " % len(plain)), line
    comp = (tmp_path / "out.z").read_bytes()
    assert len(comp) == int(line.split()[2])
    wbits = {0: -w, 1: w, 2: 16 + w}[wrap]
    assert wc.reader(wbits, comp) == (plain, True, b"")
    if wrap == 1:
        z = zlib.compressobj(6, zlib.DEFLATED, w)
        assert comp[:2] == (z.compress(b"abc") + z.flush())[:2]
        if w > 9:
            with pytest.raises(zlib.error, match="invalid window size"):
                wc.reader(w - 1, comp)


@pytest.mark.gpu
def test_set_dictionary_at_window_9(driver, tmp_path):
    """a 1000-byte dictionary, of which a 512-byte window keeps the tail: the plaintext begins with its last 200 bytes, so the
    reader needs that dictionary"""
    rng = np.random.default_rng(0x9D1C)
    zdict = rng.integers(1, 256, size=1000, dtype=np.uint8).tobytes()
    plain = zdict[-200:] + synth.silesia_like(1 << 20, seed=72).tobytes()
    (tmp_path / "in.bin").write_bytes(zdict + plain)
    line = run_driver(driver, "d", 6, 0, 9, 700001, 1000, tmp_path / "in.bin", tmp_path / "out.z")
    assert line.startswith("device %d " % len(plain)), line
    comp = (tmp_path / "out.z").read_bytes()
    assert wc.reader(-9, comp, zdict=zdict) == (plain, True, b"")
    with pytest.raises(zlib.error, match="invalid distance too far back"):
        wc.reader(-9, comp)


@pytest.mark.gpu
def test_get_dictionary_returns_at_most_the_window(driver, tmp_path):
    """deflateGetDictionary into a 512-byte buffer behind a canary: the last 512 bytes fed (deflate.c:523-529), canary intact"""
    plain = synth.silesia_like(700001, seed=73).tobytes()
    (tmp_path / "in.bin").write_bytes(plain)
    assert run_driver(driver, "g", 9, 512, tmp_path / "in.bin", tmp_path / "dict.bin") == "dict 512 canary ok"
    assert (tmp_path / "dict.bin").read_bytes() == plain[-512:]
    # a short stream: everything that was fed, no more
    (tmp_path / "short.bin").write_bytes(plain[:300])
    assert run_driver(driver, "g", 9, 512, tmp_path / "short.bin", tmp_path / "dict2.bin") == "dict 300 canary ok"
    assert (tmp_path / "dict2.bin").read_bytes() == plain[:300]
