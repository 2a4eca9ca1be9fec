"""Build check (no GPU): the front end of the Z_RLE / Z_HUFFMAN_ONLY strategies (rle_rows_kernel, deflate_rle.h) and the
forced-static block emitter of Z_FIXED compile for gfx950 without scratch memory, spills or out-of-line calls."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zlib-ng_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_strategy_kernels_no_scratch_no_calls():
    tmp = tempfile.mkdtemp(prefix="zng_isa_")
    try:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", out, os.path.join(CSRC, "deflate_dyn.hip")], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert "s_swappc_b64" not in text, "a device function or lambda is called out of line"
    kernels = {}
    for entry in text.split("\n  - .agpr_count")[1:]:               # one metadata entry per kernel
        name = re.search(r"\.name:\s*(\S+)", entry).group(1)
        kernels[name] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.vgpr_spill_count:\s*(\d+)", entry).group(1)),
                         int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", entry).group(1)))
    wanted = [k for k in kernels if "rle_rows_kernelILb" in k or "emit_dynamic_kernelILb1" in k]
    assert len(wanted) == 3, sorted(kernels)
    for k in wanted:
        scratch, spills, lds = kernels[k]
        assert scratch == 0 and spills == 0, (k, scratch, spills)
        if "rle_rows" in k:
            assert lds <= 80 * 1024, (k, lds)                          # at least two workgroups per CU
