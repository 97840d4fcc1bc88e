"""
The kernels that exaspim_label_overlaps adds, in the code-object metadata of the in-tree library (no GPU needed, in
the manner of test_kernel_budget_blocks.py): overlaps_add and the two scan instantiations over UsedPair are there
once each, built for gfx950 wave64 and bound at 256 threads, none uses scratch memory or spills, overlaps_add holds
its 2048-slot table of 12 bytes per slot and the two spill words in LDS (the scans hold block_exclusive's four wave
sums, as every instantiation does), the registers stay within the bounds DESIGN 6u writes next to the built
counts, and the new names hide no kernel that was there before.
"""

import os
import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = open(os.path.join(ROOT, "aind_exaspim_neuron_segmentation_amd", "csrc", "overlaps.hip")).read()
LDS_SLOTS = int(re.search(r"constexpr int kOvSlots = (\d+);", SOURCE).group(1))

# name -> (LDS bytes, VGPR bound); built: 43, 32 and 21 registers
NEW_KERNELS = {"overlaps_add": (LDS_SLOTS * 12 + 8, 48),
               "scan_count<exaspim::(anonymous namespace)::UsedPair>": (16, 40),
               "scan_assign<exaspim::(anonymous namespace)::UsedPair>": (16, 32)}
OLDER_KERNELS = ["tile_graph<float>", "seam_graph", "retarget", "retarget_sizes"]


def _of(kernels, name):      # noqa: F811
    out = {n: k for n, k in kernels.items() if re.search(r"\b" + re.escape(name) + r"\(", n) and "exaspim::" in n}
    assert out, name
    return out


@pytest.mark.parametrize("name", sorted(NEW_KERNELS))
def test_kernel_is_wave64_without_scratch_or_spills(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".wavefront_size"] == 64, full
    assert k[".private_segment_fixed_size"] == 0, full
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full


@pytest.mark.parametrize("name", sorted(NEW_KERNELS))
def test_kernel_is_bound_at_256_threads(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".max_flat_workgroup_size"] == 256, full


@pytest.mark.parametrize("name", sorted(NEW_KERNELS))
def test_lds_and_registers(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    lds, registers = NEW_KERNELS[name]
    assert k[".group_segment_fixed_size"] == lds, full
    assert k[".vgpr_count"] <= registers, (full, k[".vgpr_count"])


def test_six_workgroups_of_the_add_kernel_fit_a_compute_unit():
    """24 584 bytes of LDS per workgroup, 160 KiB per compute unit."""
    assert LDS_SLOTS == 2048 and 160 * 1024 // NEW_KERNELS["overlaps_add"][0] == 6


@pytest.mark.parametrize("name", OLDER_KERNELS + sorted(NEW_KERNELS))
def test_every_name_matches_exactly_one_kernel(kernels, name):      # noqa: F811
    """The budget tests find kernels by name after a word boundary and demand exactly one match."""
    assert len(_of(kernels, name)) == 1, name
