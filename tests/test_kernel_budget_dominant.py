"""
The kernels of dominant.hip in the code-object metadata of the in-tree library (no GPU needed, in the
manner of test_kernel_budget_dbf.py): the three of its own are there, built for gfx950 wave64 with 256
threads, and neither they nor the shared passes of graph_contract.h use scratch memory -- they are
memory-bound passes whose registers are a few indices and the four words of two 128-bit products.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

OWN_KERNELS = ["dominant_choose", "dominant_mark_ties", "dominant_resolve"]
SHARED_KERNELS = ["finish_map", "contract"]      # graph_contract.h: one copy each in premerge.hip and here


def _of(kernels, name):      # noqa: F811
    out = {n: k for n, k in kernels.items() if re.search(r"\b" + name + r"\(", n) and "exaspim::" in n}
    assert out, name
    return out


@pytest.mark.parametrize("name", OWN_KERNELS + SHARED_KERNELS)
def test_kernel_is_wave64_without_scratch(kernels, name):      # noqa: F811
    found = _of(kernels, name)
    assert name in SHARED_KERNELS or len(found) == 1, list(found)
    for full, k in found.items():
        assert k[".wavefront_size"] == 64, full
        assert k[".private_segment_fixed_size"] == 0, full
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full
        assert k[".max_flat_workgroup_size"] == 256, full
        assert k[".group_segment_fixed_size"] == 0, full      # no LDS: nothing is shared inside a workgroup
        assert k[".vgpr_count"] <= 64, full                   # eight waves per SIMD
