"""Build check (no GPU): the kernels of the inflate index -- the span form of the one-wavefront engine (inflate_dev.hip,
inflate_streams_span_kernel: the shared body a third time), and the window-gather and slices kernels (inflate_index.hip) with
the shared mover (bgzf_copy.h) inlined -- compile for gfx950 without scratch memory, VGPR spills or out-of-line calls; the
span kernel takes exactly the LDS of the dictionary kernel in the same assembly (the same tables and ring, so as many waves
per CU), and the two movers take none and use 16-byte vector loads and stores."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib-ng_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KEYS = ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size", "max_flat_workgroup_size")


def assembly(source):
    tmp = tempfile.mkdtemp(prefix="zng_isa_")
    try:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", out, os.path.join(CSRC, source)], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = {}
    for entry in text.split("\n  - .agpr_count")[1:]:                   # one metadata entry per kernel
        name = re.search(r"\.name:\s*(\S+)", entry).group(1)
        kernels[name] = tuple(int(re.search(r"\.%s:\s*(\d+)" % key, entry).group(1)) for key in KEYS)
    return text, kernels


def one(kernels, name):
    hit = {k: v for k, v in kernels.items() if name in k}
    assert len(hit) == 1, (name, sorted(kernels))
    return list(hit.values())[0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_span_kernel():
    text, kernels = assembly("inflate_dev.hip")
    assert "s_swappc_b64" not in text, "a device function or lambda is called out of line"
    span, dict_ = one(kernels, "inflate_streams_span_kernel"), one(kernels, "inflate_streams_dict_kernel")
    assert span[:2] == (0, 0) and span[3] == 64, span
    assert span[2] == dict_[2] and span[2] > 0, (span, dict_)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_window_and_slices_kernels():
    text, kernels = assembly("inflate_index.hip")
    assert "s_swappc_b64" not in text, "a device function or lambda is called out of line"
    for name in ("index_windows_kernel", "index_slices_kernel"):
        assert one(kernels, name) == (0, 0, 0, 256), (name, kernels)
        body = text.split(name, 1)[1].split("s_endpgm", 1)[0]
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name
    assert len(kernels) == 2, sorted(kernels)
