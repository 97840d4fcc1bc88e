"""
Register / scratch / LDS budget of the bf16x3 convolution with the fused head (conv3x3x3_x3_head,
1 .. 4 outputs), read from the code-object metadata of the in-tree library like
test_bf16x3_budget.py does for its siblings: every instantiation exists, none uses scratch, at
most 256 registers (two waves per SIMD) and two workgroups' LDS per CU.
"""

import re

from test_kernel_budget import LDS_PER_CU, kernels  # noqa: F401  (the fixture)


def test_bf16x3_head_kernels_exist_and_fit_their_occupancy_without_spills(kernels):  # noqa: F811
    sel = {}
    for name, k in kernels.items():
        m = re.search(r"conv3x3x3_x3_head<(\d+)>", name)
        if m:
            sel[int(m.group(1))] = (name, k)
    assert sorted(sel) == [1, 2, 3, 4], sorted(kernels)
    for oc, (name, k) in sorted(sel.items()):
        print(f"{name}: vgpr {k['.vgpr_count']}, lds {k['.group_segment_fixed_size']}")
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] <= 256, name
        assert 2 * k[".group_segment_fixed_size"] <= LDS_PER_CU, name


def test_the_head_variant_is_not_counted_among_the_plain_kernels(kernels):  # noqa: F811
    """test_bf16x3_budget.py selects r"conv3x3x3_x3<": the head variant has a name of its own."""
    assert not any(re.search(r"conv3x3x3_x3<", n) and "head" in n for n in kernels)
