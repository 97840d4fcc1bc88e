"""Budget of the row-mode z-column kernel with rows carried along y on top of the carried planes
(conv3x3x3_zpipe_rowzy, ConvCarryY: three carry destinations): the limits of its twins conv3x3x3_zpipe_row and
conv3x3x3_zpipe_rowz, whose body it shares -- at most 256 VGPRs (two workgroups per CU), no spills, no scratch,
the twins' LDS -- and the twins keep their figures."""
import re

from test_kernel_budget import LDS_PER_CU, kernels  # noqa: F401  (module-scoped fixture)


def test_y_carry_kernels_stay_inside_the_row_budget(kernels):  # noqa: F811
    sel = {n: k for n, k in kernels.items() if "conv3x3x3_zpipe_rowzy<" in n}
    assert len(sel) == 4, sorted(sel)         # {F16, BF16} x {6, 4}-plane tiles
    for name, k in sel.items():
        m = re.search(r"(<exaspim::(?:F16|BF16)Tag, [46], 8, 16, 2, 4>)", name)
        assert m, name
        twin = [t for n, t in kernels.items() if "conv3x3x3_zpipe_rowz" + m.group(1) in n]
        assert len(twin) == 1, name
        assert k[".vgpr_count"] <= 256, name
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".group_segment_fixed_size"] == twin[0][".group_segment_fixed_size"], name
        assert 2 * k[".group_segment_fixed_size"] <= LDS_PER_CU, name
        # ConvArgs keeps its size: the y fields travel in a second argument of this symbol only
        sizes = [a[".size"] for a in k[".args"] if a.get(".value_kind") == "by_value"]
        assert sizes[0] == 184 and sizes[1] == 48, (name, sizes)
        assert [a[".size"] for a in twin[0][".args"] if a.get(".value_kind") == "by_value"][0] == 184, name
