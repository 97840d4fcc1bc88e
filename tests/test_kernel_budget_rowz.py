"""Budget of the row-mode z-column kernel with carried planes (conv3x3x3_zpipe_rowz, ConvArgs::in_z0 ..
out_shift): the limits of conv3x3x3_zpipe_row, whose body it shares -- at most 256 VGPRs (two workgroups
per CU), no spills, no scratch, LDS for two workgroups."""
import re

from test_kernel_budget import LDS_PER_CU, kernels  # noqa: F401  (module-scoped fixture)


def test_carry_kernels_stay_inside_the_row_budget(kernels):  # noqa: F811
    sel = {n: k for n, k in kernels.items() if "conv3x3x3_zpipe_rowz<" in n}
    assert len(sel) == 4, sorted(sel)         # {F16, BF16} x {6, 4}-plane tiles
    for name, k in sel.items():
        assert re.search(r"(F16|BF16)Tag, [46], 8, 16, 2, 4>", name), name
        assert k[".vgpr_count"] <= 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert 2 * k[".group_segment_fixed_size"] <= LDS_PER_CU, name
