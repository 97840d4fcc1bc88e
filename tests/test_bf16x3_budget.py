"""
Register / scratch / LDS budget of the bf16x3 convolution kernel (conv3x3x3_x3), read from the
code-object metadata of the in-tree library like test_kernel_budget.py does for its siblings: no
scratch, at most 256 registers (two waves per SIMD) and two workgroups' LDS per CU.
"""

import re

from test_kernel_budget import LDS_PER_CU, kernels  # noqa: F401  (the fixture)


def test_bf16x3_kernels_fit_their_occupancy_without_spills(kernels):  # noqa: F811
    sel = {n: k for n, k in kernels.items() if re.search(r"conv3x3x3_x3<", n)}
    assert len(sel) >= 10, sorted(sel)
    for name, k in sel.items():
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 256, name
        assert 2 * k[".group_segment_fixed_size"] <= LDS_PER_CU, name
