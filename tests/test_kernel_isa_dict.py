"""Build check (no GPU) of the kernels of the shared preset dictionary: metadata only -- scratch, VGPR spills, LDS and the
out-of-line call marker tests/test_kernel_isa.py looks for.

  deflate_quick_dict_kernel    the dictionary form of the level-1 kernel: four waves per stream and no more LDS than
                               deflate_quick_kernel, so eight workgroups per CU still fit
  inflate_streams_dict_kernel  the dictionary form of the stream inflater: no more LDS than the ring-4096 stream form
  dict_head_kernel             the primed head table (dict.hip)
  frame_compress_kernel, parse_header_kernel, verify_trailer_kernel   the wrapper kernels, which write and judge the 16-byte
                               FDICT wrapper as well (framing_dev.hip)"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib-ng_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _kernels(source):
    tmp = tempfile.mkdtemp(prefix="zng_isa_")
    try:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", out, os.path.join(CSRC, source)], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert "s_swappc_b64" not in text, source + ": a device function or lambda is called out of line"
    kernels = {}
    for entry in text.split("\n  - .agpr_count")[1:]:               # one metadata entry per kernel
        name = re.search(r"\.name:\s*(\S+)", entry).group(1)
        kernels[name] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.vgpr_spill_count:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.max_flat_workgroup_size:\s*(\d+)", entry).group(1)))
    return kernels


def _one(kernels, part):
    hit = {k: v for k, v in kernels.items() if part in k}
    assert len(hit) == 1, (part, sorted(kernels))
    (value,) = hit.values()
    return value


def test_deflate_dictionary_form():
    kernels = _kernels("deflate_stream.hip")
    scratch, spills, lds, wg = _one(kernels, "deflate_quick_dict_kernel")
    _, _, lds_plain, wg_plain = _one(kernels, "20deflate_quick_kernel")
    assert scratch == 0 and spills == 0, (scratch, spills)
    assert wg == 256 and wg_plain == 256                              # four waves per stream
    assert 0 < lds <= lds_plain, (lds, lds_plain)
    assert 8 * lds <= 160 << 10                                       # eight workgroups in a CU's 160 KiB


def test_inflate_dictionary_form():
    kernels = _kernels("inflate_dev.hip")
    scratch, spills, lds, wg = _one(kernels, "inflate_streams_dict_kernelILi4096E")
    _, _, lds_plain, wg_plain = _one(kernels, "inflate_streams_kernelILi4096ELb0ELb0ELb0E")
    assert scratch == 0 and spills == 0, (scratch, spills)
    assert wg == 64 and wg_plain == 64
    assert 0 < lds <= lds_plain, (lds, lds_plain)


def test_head_table_and_framing_kernels():
    head = _kernels("dict.hip")
    assert len(head) == 1, sorted(head)
    assert _one(head, "dict_head_kernel") == (0, 0, 0, 256)
    framing = _kernels("framing_dev.hip")
    for name in ("frame_compress_kernel", "parse_header_kernel", "verify_trailer_kernel"):
        scratch, spills, lds, wg = _one(framing, name)
        assert (scratch, spills, lds, wg) == (0, 0, 0, 256), (name, scratch, spills, lds, wg)
