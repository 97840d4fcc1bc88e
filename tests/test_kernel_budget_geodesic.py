"""
The kernels of exaspim_geodesic_begin / _sweeps / _farthest in the code-object metadata of the in-tree
library (no GPU needed, in the manner of test_kernel_budget_dbf.py): they are there, built for gfx950 wave64,
none uses scratch memory or spills, the multi-thread ones are bound at 256 threads, and the sweep kernel in
both of its modes keeps its tile, halo included, within 32 KiB of LDS, so that five workgroups fit the
160 KiB of a CU.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

SWEEPS = ["geodesic_sweep<true>", "geodesic_sweep<false>"]
BOUND_KERNELS = ["geodesic_init", "geodesic_sources", "far_init", "far_pass", "far_finish"] + SWEEPS
ALL_KERNELS = BOUND_KERNELS + ["geodesic_publish"]


def _of(kernels, name):      # noqa: F811
    out = {n: k for n, k in kernels.items() if re.search(r"\b" + re.escape(name) + r"\(", n) and "exaspim::" in n}
    assert out, name
    return out


@pytest.mark.parametrize("name", ALL_KERNELS)
def test_kernel_is_wave64_without_scratch_or_spills(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".wavefront_size"] == 64, full
    assert k[".private_segment_fixed_size"] == 0, full
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full


@pytest.mark.parametrize("name", BOUND_KERNELS)
def test_kernel_is_bound_at_256_threads(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".max_flat_workgroup_size"] == 256, full


@pytest.mark.parametrize("name", SWEEPS)
def test_the_sweep_fits_five_workgroups_into_a_cu(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    lds = k[".group_segment_fixed_size"]
    assert 10 * 10 * 34 * 8 <= lds <= 32 * 1024, (full, lds)      # labels and field with the halo, little else
    assert 5 * lds <= 160 * 1024


@pytest.mark.parametrize("name", ["geodesic_init", "geodesic_sources", "far_init", "far_pass", "far_finish"])
def test_the_plain_passes_use_no_lds(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".group_segment_fixed_size"] == 0, full
    assert k[".vgpr_count"] <= 64, full
