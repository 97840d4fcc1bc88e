"""Budget of the row-mode border kernels with carried planes (conv3x3x3_t14_borders_carry, kRowStageBordersCarry):
no scratch and no register spilled to memory, at most the VGPRs and the LDS of the conv3x3x3_t14 border
instantiation (ZORD and POOL, the TZ x 16 x 2 tile) whose body each shares -- four workgroups per CU.

(The uncarried twins keep 16 - 17 scalar registers in lanes of a vector register, `.sgpr_spill_count`; the carried
kernels 23 - 24, for the carry fields. Those cost no memory traffic: the scratch size below is zero.)"""
import re

from test_kernel_budget import kernels  # noqa: F401  (module-scoped fixture)


def test_border_carry_kernels_stay_inside_their_twins_budget(kernels):  # noqa: F811
    sel = {n: k for n, k in kernels.items() if "conv3x3x3_t14_borders_carry<" in n}
    assert len(sel) == 4, sorted(sel)         # {F16, BF16} x the two depths launch_row_borders picks
    seen = set()
    for name, k in sel.items():
        m = re.search(r"conv3x3x3_t14_borders_carry<(.*(?:F16|BF16)Tag), (8, 2|4, 1)>", name)
        assert m, name
        seen.add((m.group(1), m.group(2)))
        tz, mt = m.group(2).split(", ")
        twin = [t for t in kernels
                if f"conv3x3x3_t14<{m.group(1)}, {tz}, 16, 2, 4, 1, {mt}, 1, 4, 3, true, true>" in t]
        assert len(twin) == 1, (name, twin)
        t = kernels[twin[0]]
        assert k[".vgpr_spill_count"] == 0, name
        assert k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= t[".vgpr_count"] <= 128, name
        assert k[".group_segment_fixed_size"] <= t[".group_segment_fixed_size"], name
    assert len(seen) == 4
