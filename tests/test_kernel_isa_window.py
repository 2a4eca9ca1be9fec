"""Build check (no GPU): the window form of the rows matcher (lz_rows_win_kernel, deflate_dyn.hip: the body of lz_rows_kernel
with the distance cap and the priming length as arguments) needs no more of the CU than lz_rows_kernel in the same build -- no
more scratch, no more spilled registers, no more LDS.  One workgroup of 1024 lanes per CU at 160 KiB of LDS is the design of both;
a form that spilled or grew would still run, and slowly.  hipcc cross-compiles here, as tests/test_kernel_isa.py does."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib-ng_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")


def _kernel_metadata(text):
    """{kernel name: {field: int}} from the amdhsa.kernels list of the assembly's metadata"""
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s*(\S+)", entry, flags=re.M)        # (an argument's own .name is indented further)
        if name:                                           # (the lists behind the kernels -- the version -- have none)
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s*(\d+)\s*$", entry, flags=re.M)}
    return out


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tempfile.mkdtemp(prefix="zng_isa_win_")
    try:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", out, os.path.join(CSRC, "deflate_dyn.hip")], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return _kernel_metadata(open(out).read())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _one(kernels, fragment):
    names = [n for n in kernels if fragment in n]
    assert len(names) == 1, (fragment, names)
    return kernels[names[0]]


def test_window_form_needs_no_more_than_the_plain_kernel(kernels):
    plain, win = _one(kernels, "lz_rows_kernel"), _one(kernels, "lz_rows_win_kernel")
    print("lz_rows_kernel     %r" % {k: plain[k] for k in FIELDS + ("sgpr_count", "vgpr_count", "sgpr_spill_count")})
    print("lz_rows_win_kernel %r" % {k: win[k] for k in FIELDS + ("sgpr_count", "vgpr_count", "sgpr_spill_count")})
    for k in FIELDS:
        assert win[k] <= plain[k], (k, win[k], plain[k])
    assert win["group_segment_fixed_size"] <= 160 * 1024


def test_window_form_takes_cap_and_window_as_arguments(kernels):
    """the two 32-bit arguments behind lz_rows_kernel's own: 8 more bytes of kernel arguments, nothing else"""
    plain, win = _one(kernels, "lz_rows_kernel"), _one(kernels, "lz_rows_win_kernel")
    assert win["kernarg_segment_size"] == plain["kernarg_segment_size"] + 8
