"""Build check (no GPU): the kernels of zng_rocm_inflate_sizes_dev / zng_rocm_uncompress_packed_dev (inflate_sizes.hip) compile
for gfx950 without scratch memory, VGPR spills or out-of-line calls, as the stream kernel they were cut from must
(tests/test_kernel_isa_batch.py holds the rule), and the sizing kernel's tables -- no ring -- leave room for more than the
decoder's 16 wavefronts per CU."""
import os

import pytest

from test_kernel_isa_batch import HIPCC, LDS_PER_CU, _clean, _kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sizing_and_packing_kernels():
    kernels = _kernels("inflate_sizes.hip")
    sizing = _clean(kernels, r"inflate_sizes_kernel", 1)
    for name in ("sizes_place_kernel", "sizes_patch_kernel", "sizes_final_kernel"):
        _clean(kernels, name, 1)
    (_, _, lds), = sizing.values()
    assert 0 < lds * 20 <= LDS_PER_CU, lds
