"""Budget of the level-1 convolution kernels with carried planes (conv3x3x3_t14_carry, ConvArgs::in_z0 ..
out_shift): no scratch and no spills, at most the VGPRs and exactly the LDS of the conv3x3x3_t14 instantiation
whose body each shares (two workgroups per CU)."""
import re

from test_kernel_budget import kernels  # noqa: F401  (module-scoped fixture)


def test_carry_kernels_stay_inside_their_twins_budget(kernels):  # noqa: F811
    sel = {n: k for n, k in kernels.items() if "conv3x3x3_t14_carry<" in n}
    assert len(sel) == 4, sorted(sel)         # {F16, BF16} x {down1.0, down1.3 with its max-pool}
    for name, k in sel.items():
        m = re.search(r"conv3x3x3_t14_carry<(.*(?:F16|BF16)Tag), 4, 8, 16, 4, 1, 4, 2, 2, 3, (false|true)>", name)
        assert m, name
        twin = [t for t in kernels
                if f"conv3x3x3_t14<{m.group(1)}, 4, 8, 16, 4, 1, 4, 2, 2, 3, false, {m.group(2)}>" in t]
        assert len(twin) == 1, (name, twin)
        t = kernels[twin[0]]
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, name
        assert k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= t[".vgpr_count"] <= 256, name
        assert k[".group_segment_fixed_size"] == t[".group_segment_fixed_size"], name
