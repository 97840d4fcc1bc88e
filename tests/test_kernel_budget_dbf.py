"""
The kernels of dbf.hip in the code-object metadata of the in-tree library (no GPU needed, in the manner
of test_kernel_budget.py): all five are there, built for gfx950 wave64, and none of them uses scratch
memory -- they are memory-bound passes whose registers are a handful of indices.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

DBF_KERNELS = ["dbf_x", "dbf_axis", "table_init", "table_pass", "table_finish"]


def _of(kernels, name):      # noqa: F811
    out = {n: k for n, k in kernels.items() if re.search(r"\b" + name + r"\(", n) and "exaspim::" in n}
    assert out, name
    return out


@pytest.mark.parametrize("name", DBF_KERNELS)
def test_kernel_is_wave64_without_scratch(kernels, name):      # noqa: F811
    for full, k in _of(kernels, name).items():
        assert k[".wavefront_size"] == 64, full
        assert k[".private_segment_fixed_size"] == 0, full
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full
        assert k[".max_flat_workgroup_size"] == 256, full


def test_four_workgroups_of_the_x_pass_fit_a_cu(kernels):      # noqa: F811
    """Its LDS is the table of chunk carries of the longest row the diagonal bound admits."""
    (k,) = _of(kernels, "dbf_x").values()
    assert k[".group_segment_fixed_size"] <= 1024
    for name, lds in (("dbf_axis", 0), ("table_pass", 8192)):      # table_pass: the workgroup's pool of counts
        (k,) = _of(kernels, name).values()
        assert k[".group_segment_fixed_size"] <= lds, name
        assert k[".vgpr_count"] <= 64, name      # eight waves per SIMD
