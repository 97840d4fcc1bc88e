"""
The kernels of exaspim_fill_holes in the code-object metadata of the in-tree library (no GPU needed, in the
manner of test_kernel_budget_dbf.py): the mask kernel in both of its forms, the two survey passes and the
fill are there, built for gfx950 wave64 with 256 threads, and none of them uses scratch memory or spills --
they are memory-bound passes whose registers are a handful of indices.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

HOLES_KERNELS = ["edge_mask_background<4>", "edge_mask_background<1>", "survey_faces", "survey", "fill"]


def _of(kernels, name):      # noqa: F811
    out = {n: k for n, k in kernels.items() if re.search(r"\b" + re.escape(name) + r"\(", n) and "exaspim::" in n}
    assert out, name
    return out


@pytest.mark.parametrize("name", HOLES_KERNELS)
def test_kernel_is_wave64_without_scratch(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".wavefront_size"] == 64, full
    assert k[".private_segment_fixed_size"] == 0, full
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full
    assert k[".max_flat_workgroup_size"] == 256, full


@pytest.mark.parametrize("name", HOLES_KERNELS)
def test_kernel_keeps_eight_waves_per_simd_and_no_lds(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".vgpr_count"] <= 64, full
    assert k[".group_segment_fixed_size"] == 0, full
