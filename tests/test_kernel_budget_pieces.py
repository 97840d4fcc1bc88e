"""
The kernels of exaspim_label_pieces in the code-object metadata of the in-tree library (no GPU needed, in the manner
of test_kernel_budget_border.py): they are there, built for gfx950 wave64, none uses scratch memory or spills, all
are bound at 256 threads, the tile pass holds the tile's labels, parents and counts and one flag per wave in LDS
(3 * 8192 + 16 bytes) and the other passes none, the registers stay within the bounds DESIGN 6q writes
next to the built counts, and the new names hide no kernel that was there before.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

# name -> (LDS bytes, VGPR bound); built: 96, 22, 8 and 14 registers
NEW_KERNELS = {"pieces_tile_pass": (3 * 8192 + 16, 112), "pieces_seam_merge": (0, 32), "pieces_sizes": (0, 16),
               "pieces_relabel": (0, 24)}
NEW_SCANS = ["scan_count<exaspim::(anonymous namespace)::PieceRoot>",
             "scan_assign<exaspim::(anonymous namespace)::PieceRoot>"]
OLDER_KERNELS = ["tile_pass", "face_merge", "flatten", "sizes", "relabel", "survey_faces", "survey", "fill",
                 "seam_mark", "seam_union", "border_union", "table_flatten"]


def _of(kernels, name):      # noqa: F811
    out = {n: k for n, k in kernels.items() if re.search(r"\b" + re.escape(name) + r"\(", n) and "exaspim::" in n}
    assert out, name
    return out


@pytest.mark.parametrize("name", sorted(NEW_KERNELS) + NEW_SCANS)
def test_kernel_is_wave64_without_scratch_or_spills(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".wavefront_size"] == 64, full
    assert k[".private_segment_fixed_size"] == 0, full
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full


@pytest.mark.parametrize("name", sorted(NEW_KERNELS) + NEW_SCANS)
def test_kernel_is_bound_at_256_threads(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    assert k[".max_flat_workgroup_size"] == 256, full


@pytest.mark.parametrize("name", sorted(NEW_KERNELS))
def test_lds_and_registers(kernels, name):      # noqa: F811
    (full, k), = _of(kernels, name).items()
    lds, registers = NEW_KERNELS[name]
    assert k[".group_segment_fixed_size"] == lds, full
    assert k[".vgpr_count"] <= registers, (full, k[".vgpr_count"])


def test_the_tile_pass_keeps_four_workgroups_on_a_cu(kernels):      # noqa: F811
    """At most 128 registers are four waves per SIMD, and 24592 bytes are six workgroups' LDS."""
    (full, k), = _of(kernels, "pieces_tile_pass").items()
    assert 4 * k[".vgpr_count"] <= 512 and 4 * k[".group_segment_fixed_size"] <= 160 * 1024, full


@pytest.mark.parametrize("name", OLDER_KERNELS + sorted(NEW_KERNELS) + NEW_SCANS)
def test_every_name_matches_exactly_one_kernel(kernels, name):      # noqa: F811
    """The budget tests find kernels by name after a word boundary and demand exactly one match."""
    assert len(_of(kernels, name)) == 1, name
