"""Shared by the deflateCopy / inflateCopy tests (test_coarse_copy_cpu.py, test_gpu_coarse_copy.py): the inputs, the build of
tests/c/coarse_copy_driver.c -- against libzng_rocm.so, or against the CPU stand-in tests/c/hook_stub.cpp plus the
project's host decoder -- and the reading of what the driver prints."""
import functools
import importlib
import os
import subprocess
import zlib

import numpy as np

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = os.path.join(ROOT, "integration", "arch", "rocm")
DEFINES = ["-DZNG_ROCM_STANDALONE_CHECK", "-DROCM_MIN_BYTES=1024", "-DROCM_INFLATE_MIN_BYTES=1",
           "-DROCM_DEFLATE_BLOCK_BYTES=1048576"]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "c"), "-I" + ARCH]
C_FLAGS = ["-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2"]
C_SOURCES = [os.path.join(ROOT, "tests", "c", "coarse_copy_driver.c")] + \
            [os.path.join(ARCH, f) for f in ("rocm_deflate.c", "rocm_inflate.c", "rocm_slots.c", "rocm_features.c")]
GATHERED = 300000                       # the driver's "gather" point


@functools.lru_cache(maxsize=None)
def inputs():
    """P, A, B: the plaintext up to the copy point ends with 20000 random bytes R; the source's tail is R again and the
    copy's is R rotated by half, so both tails lie whole in the last 32 KiB of P"""
    r = np.random.default_rng(20261020).integers(0, 256, 20000, dtype=np.uint8).tobytes()
    return synth.silesia_like(1536 << 10, seed=41).tobytes() + r, r, r[10000:] + r[:10000]


@functools.lru_cache(maxsize=None)
def zstream():
    return zlib.compress(inputs()[0], 6)


def build_driver(workdir, stub):
    """the driver and the adapters as strict C11; stub=False links libzng_rocm.so, stub=True the CPU stand-in"""
    workdir = str(workdir)
    exe = os.path.join(workdir, "coarse_copy_driver_stub" if stub else "coarse_copy_driver")
    if not stub:
        zr = importlib.import_module("zlib-ng_amd")
        libdir = os.path.dirname(zr.lib_path())
        subprocess.check_call(["gcc"] + C_FLAGS + DEFINES + INCLUDES + C_SOURCES +
                              ["-o", exe, "-L" + libdir, "-lzng_rocm", "-Wl,-rpath," + libdir])
        return exe
    objs = []
    for src in C_SOURCES:
        obj = os.path.join(workdir, os.path.basename(src) + ".o")
        subprocess.check_call(["gcc"] + C_FLAGS + DEFINES + INCLUDES + ["-c", src, "-o", obj])
        objs.append(obj)
    for src, flags in ((os.path.join(ROOT, "tests", "c", "hook_stub.cpp"), ["-Wall", "-Wextra", "-Werror"]),
                       (os.path.join(ROOT, "zlib-ng_amd", "csrc", "inflate_host.cpp"), [])):
        obj = os.path.join(workdir, os.path.basename(src) + ".o")
        subprocess.check_call(["g++", "-std=c++17", "-O2"] + flags + INCLUDES + ["-c", src, "-o", obj])
        objs.append(obj)
    subprocess.check_call(["g++"] + objs + ["-pthread", "-o", exe])
    return exe


def run(exe, *args, env=None):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env) if env else None)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])
    return p.stdout.splitlines()


def parse(lines):
    """{'at_copy': {'in_len': .., 'owed': .., ...}, 'src': [words], 'copy': [words], 'failed': code or None, 'live': n}"""
    res = {"failed": None, "src": None, "copy": None}
    for line in lines:
        words = line.split()
        if words[0] == "copy" and words[1].startswith("in_len="):
            res["at_copy"] = {k: int(v) for k, v in (w.split("=") for w in words[1:])}
        elif words[0] == "copy" and words[1] == "failed":
            res["failed"] = int(words[2])
        elif words[0] in ("src", "copy"):
            res[words[0]] = line.split(None, 1)[1]
        elif words[0] == "live":
            res["live"] = int(words[1])
    return res


def write_inputs(tmp_path):
    p, a, b = inputs()
    for name, data in (("P", p), ("A", a), ("B", b)):
        (tmp_path / name).write_bytes(data)


def deflate_copy(exe, tmp_path, point, order, level=6, wrap=1, w_bits=15, strategy=0, env=None):
    """one run of the driver's deflate side -> (parsed output, source's bytes, copy's bytes)"""
    write_inputs(tmp_path)
    res = parse(run(exe, "d", level, wrap, w_bits, strategy, point, order, tmp_path / "P", tmp_path / "A", tmp_path / "B",
                    tmp_path / "src.z", tmp_path / "copy.z", env=env))
    assert res["live"] == 0, res
    read = lambda name: (tmp_path / name).read_bytes() if (tmp_path / name).exists() else None
    return res, read("src.z"), read("copy.z")


def inflate_zlib(data, wrap):
    """CPython's zlib as the reader: header and Adler-32 trailer checked, nothing may follow the stream"""
    d = zlib.decompressobj(15 if wrap else -15)
    out = d.decompress(data)
    assert d.eof and not d.unused_data
    return out


def check_deflate_round_trip(res, src, cpy, point, wrap=1):
    """the source's output decodes to P + A, the copy's to P + B (at "finish" the tail was in before the copy: P + A)"""
    p, a, b = inputs()
    want_src, want_copy = p + a, (p + a if point == "finish" else p + b)
    assert res["failed"] is None, res
    for who, data, want in (("src", src, want_src), ("copy", cpy, want_copy)):
        words = res[who].split()
        assert words[0] == "device" and int(words[1]) == len(want) and int(words[2]) == len(data), (who, res)
        assert inflate_zlib(data, wrap) == want, who


def inflate_copy(exe, tmp_path, at, last_out=0, order=0, in_chunk=50000, stream=None, alt=None, plain_len=None, wbits=15,
                 env=None):
    """one run of the driver's inflate side -> (parsed output, source's plaintext, copy's plaintext)"""
    stream = zstream() if stream is None else stream
    (tmp_path / "in.z").write_bytes(stream)
    if alt is not None:
        assert len(alt) == len(stream)
        (tmp_path / "alt.z").write_bytes(alt)
    for name in ("src.bin", "copy.bin"):
        if (tmp_path / name).exists():
            (tmp_path / name).unlink()
    res = parse(run(exe, "i", 1, wbits, at, last_out, order, in_chunk, tmp_path / "in.z",
                    tmp_path / "alt.z" if alt is not None else "-", tmp_path / "src.bin", tmp_path / "copy.bin",
                    len(inputs()[0]) if plain_len is None else plain_len, env=env))
    assert res["live"] == 0, res
    read = lambda name: (tmp_path / name).read_bytes() if (tmp_path / name).exists() else None
    return res, read("src.bin"), read("copy.bin")


def flipped(stream, at):
    """the stream with one bit flipped half way between `at` and its end, and what CPython's zlib says about it"""
    bad = bytearray(stream)
    bad[at + (len(stream) - at) // 2] ^= 0x10
    try:
        zlib.decompress(bytes(bad))
    except zlib.error as e:
        return bytes(bad), str(e)
    raise AssertionError("the damaged stream still decodes")


# the copy points of the inflate side: (name, bytes fed before the copy as a function of the stream's length, avail_out of
# the last call before it)
def inflate_points(n):
    return {"first": (0, 0), "mid": (50000 * (4 * n // 10 // 50000), 0), "mid2": (50000 * (4 * n // 10 // 50000) + 50000, 0),
            "pending": (300000, 4096), "trailer": (n - 4, 0)}
