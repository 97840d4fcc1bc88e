"""
The kernels of exaspim_border_targets and exaspim_teasar_round_given in the code-object metadata of the in-tree
library (no GPU needed, in the manner of test_kernel_budget_fix_branching.py): they are there, built for gfx950
wave64, none uses scratch memory or spills, all are bound at 256 threads, none uses LDS (one thread
per face pixel or per label, nothing shared inside a workgroup), all stay within 32 VGPRs, and their names hide
no kernel that was there before.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

NEW_KERNELS = ["border_gather", "border_axis", "border_union", "border_peaks", "border_emit", "teasar_given_lengths"]
OLDER_KERNELS = ["dbf_x", "dbf_axis", "table_init", "table_pass", "table_finish", "teasar_init", "teasar_round_init",
                 "teasar_targets", "teasar_branch_lengths", "teasar_branch_write", "teasar_invalidate<true>",
                 "teasar_invalidate<false>", "reseed_clear", "reseed_seeds", "hops_seed_list", "far_pass"]


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
    assert k[".vgpr_count"] <= 32, full      # a few indices per thread, bound by memory latency


@pytest.mark.parametrize("name", OLDER_KERNELS + NEW_KERNELS)
def test_every_name_matches_exactly_one_kernel(kernels, name):      # noqa: F811
    """The budget tests find kernels by name after a word boundary and demand exactly one match."""
    assert len(_of(kernels, name)) == 1, name
