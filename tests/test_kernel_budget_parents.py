"""
The kernels of exaspim_geodesic_parents_begin / _sweeps / _finish and exaspim_trace_paths in the code-object
metadata of the in-tree library (no GPU needed, in the manner of test_kernel_budget_geodesic.py): they are
there, built for gfx950 wave64, none uses scratch memory or spills, all are bound at 256 threads, the hops
sweep in both of its modes keeps its tile, halo included, within 32 KiB of LDS, so that five workgroups fit
the 160 KiB of a CU, and the plain passes use no LDS.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

SWEEPS = ["hops_sweep<true>", "hops_sweep<false>"]
PLAIN = ["hops_init", "hops_seed", "parents_pick<true>", "parents_pick<false>", "trace_paths"]
ALL_KERNELS = PLAIN + SWEEPS


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


@pytest.mark.parametrize("name", ALL_KERNELS)
def test_kernel_is_bound_at_256_threads(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".max_flat_workgroup_size"] == 256, full


@pytest.mark.parametrize("name", SWEEPS)
def test_the_sweep_fits_five_workgroups_into_a_cu(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    lds = k[".group_segment_fixed_size"]
    assert 10 * 10 * 34 * 8 <= lds <= 32 * 1024, (full, lds)      # masks and hops with the halo, little else
    assert 5 * lds <= 160 * 1024


@pytest.mark.parametrize("name", PLAIN)
def test_the_plain_passes_use_no_lds(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".group_segment_fixed_size"] == 0, full
    assert k[".vgpr_count"] <= 64, full


def test_the_new_names_hide_no_existing_kernel(kernels):      # noqa: F811
    """The budget tests find kernels by name after a word boundary and demand exactly one match."""
    for name in ("geodesic_init", "geodesic_sources", "geodesic_publish", "far_init", "far_pass", "far_finish",
                 "geodesic_sweep<true>", "geodesic_sweep<false>"):
        assert len(_of(kernels, name)) == 1, name
