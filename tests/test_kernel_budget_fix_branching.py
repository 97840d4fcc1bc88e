"""
The kernels of exaspim_geodesic_reseed and exaspim_geodesic_parents_begin_seeds in the code-object metadata of
the in-tree library (no GPU needed, in the manner of test_kernel_budget_teasar.py): they are there, built for
gfx950 wave64, none uses scratch memory or spills, all are bound at 256 threads, none uses LDS, all stay within
64 VGPRs, and their names hide no kernel that was there before.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

NEW_KERNELS = ["reseed_clear", "reseed_seeds", "hops_seed_list"]
OLDER_KERNELS = ["geodesic_init", "geodesic_sources", "geodesic_publish", "far_init", "far_pass", "far_finish",
                 "geodesic_sweep<true>", "geodesic_sweep<false>", "hops_init", "hops_seed", "hops_sweep<true>",
                 "hops_sweep<false>", "parents_pick<true>", "parents_pick<false>", "trace_paths", "teasar_init",
                 "teasar_round_init", "teasar_targets", "teasar_branch_lengths", "teasar_branch_write",
                 "teasar_invalidate<true>", "teasar_invalidate<false>"]


def _of(kernels, name):      # noqa: F811
    out = {n: k for n, k in kernels.items() if re.search(r"\b" + re.escape(name) + r"\(", n) and "exaspim::" in n}
    assert out, name
    return out


@pytest.mark.parametrize("name", NEW_KERNELS)
def test_kernel_is_wave64_without_scratch_or_spills(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".wavefront_size"] == 64, full
    assert k[".private_segment_fixed_size"] == 0, full
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full


@pytest.mark.parametrize("name", NEW_KERNELS)
def test_kernel_is_bound_at_256_threads(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".max_flat_workgroup_size"] == 256, full


@pytest.mark.parametrize("name", NEW_KERNELS)
def test_the_passes_use_no_lds_and_few_registers(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".group_segment_fixed_size"] == 0, full
    assert k[".vgpr_count"] <= 64, full      # eight waves per SIMD: the passes are bound by memory


@pytest.mark.parametrize("name", OLDER_KERNELS + NEW_KERNELS)
def test_every_name_matches_exactly_one_kernel(kernels, name):      # noqa: F811
    """The budget tests find kernels by name after a word boundary and demand exactly one match."""
    assert len(_of(kernels, name)) == 1, name
