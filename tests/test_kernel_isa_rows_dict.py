"""Build check (no GPU) of the kernels of the shared preset dictionary at every level, in deflate_dyn.hip: metadata only --
scratch, VGPR spills, LDS, workgroup size and the out-of-line call marker tests/test_kernel_isa.py looks for.

  lz_rows_dict_kernel     the dictionary form of the rows matcher: 1024 lanes per segment, no scratch, no spills and no more
                          LDS than lz_rows_kernel, so one workgroup per CU fits as before
  rows_dict_table_kernel  the primed row tables of a dictionary object: one workgroup of 1024 lanes, the same bounds"""
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


@pytest.fixture(scope="module")
def kernels():
    tmp = tempfile.mkdtemp(prefix="zng_isa_")
    try:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", out, os.path.join(CSRC, "deflate_dyn.hip")], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert "s_swappc_b64" not in text, "deflate_dyn.hip: a device function or lambda is called out of line"
    found = {}
    for entry in text.split("\n  - .agpr_count")[1:]:               # one metadata entry per kernel
        name = re.search(r"\.name:\s*(\S+)", entry).group(1)
        found[name] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", entry).group(1)),
                       int(re.search(r"\.vgpr_spill_count:\s*(\d+)", entry).group(1)),
                       int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1)),
                       int(re.search(r"\.max_flat_workgroup_size:\s*(\d+)", entry).group(1)))
    return found


def _one(kernels, part):
    hit = {k: v for k, v in kernels.items() if part in k}
    assert len(hit) == 1, (part, sorted(kernels))
    (value,) = hit.values()
    return value


def test_dictionary_form_of_the_rows_matcher(kernels):
    scratch, spills, lds, wg = _one(kernels, "lz_rows_dict_kernel")
    _, _, lds_plain, wg_plain = _one(kernels, "14lz_rows_kernel")
    assert scratch == 0 and spills == 0, (scratch, spills)
    assert wg == 1024 and wg_plain == 1024
    assert 0 < lds <= lds_plain <= 160 << 10, (lds, lds_plain)


def test_table_kernel(kernels):
    scratch, spills, lds, wg = _one(kernels, "rows_dict_table_kernel")
    _, _, lds_plain, _ = _one(kernels, "14lz_rows_kernel")
    assert scratch == 0 and spills == 0, (scratch, spills)
    assert wg == 1024
    assert 0 < lds <= lds_plain, (lds, lds_plain)
