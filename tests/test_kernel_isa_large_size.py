"""Build check (no GPU): the kernels of zng_rocm_uncompress_large_size_dev / zng_rocm_uncompress_large_sizes_dev
(inflate_large_size.hip) compile for gfx950 without scratch memory, VGPR spills or out-of-line calls, as the sizing kernel
whose text they include must (tests/test_kernel_isa_batch.py holds the rule).  They have no window and no ring: their LDS is
the sizing kernel's tables and nothing else, so more wavefronts fit a CU than the part decoder's 12 or 13."""
import os

import pytest

from test_kernel_isa_batch import HIPCC, LDS_PER_CU, _clean, _kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_counting_kernels():
    kernels = _kernels("inflate_large_size.hip")
    parts = _clean(kernels, r"inflate_size_parts_kernel", 1)
    whole = _clean(kernels, r"inflate_size_stream_kernel", 1)
    assert len(kernels) == 2, sorted(kernels)
    (_, _, lds_sizing), = _clean(_kernels("inflate_sizes.hip"), r"inflate_sizes_kernel", 1).values()
    for (_, _, lds), in (parts.values(), whole.values()):
        assert lds == lds_sizing and 0 < lds * 20 <= LDS_PER_CU, (lds, lds_sizing)
