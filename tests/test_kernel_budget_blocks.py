"""
The kernels that exaspim_label_pieces_open adds, in the code-object metadata of the in-tree library (no GPU needed, in
the manner of test_kernel_budget_pieces.py): the mark pass and the two scan instantiations over OpenPieceRoot are
there, built for gfx950 wave64 and bound at 256 threads, none uses scratch memory or spills, the mark pass uses no
LDS (the scans hold block_exclusive's four wave sums, as every instantiation does), the registers stay within the
bounds DESIGN 6r writes next to the built counts, and the new names hide no kernel that was there before.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

# name -> (LDS bytes, VGPR bound); built: 22, 34 and 21 registers
NEW_KERNELS = {"pieces_mark_open": (0, 32),
               "scan_count<exaspim::(anonymous namespace)::OpenPieceRoot>": (16, 40),
               "scan_assign<exaspim::(anonymous namespace)::OpenPieceRoot>": (16, 32)}
OLDER_KERNELS = ["tile_pass", "face_merge", "flatten", "sizes", "relabel", "survey_faces", "survey", "fill",
                 "seam_mark", "seam_union", "border_union", "border_gather", "table_flatten", "pieces_tile_pass",
                 "pieces_seam_merge", "pieces_sizes", "pieces_relabel",
                 "scan_count<exaspim::(anonymous namespace)::PieceRoot>",
                 "scan_assign<exaspim::(anonymous namespace)::PieceRoot>"]


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


def test_the_new_predicate_is_not_taken_for_the_older_one(kernels):      # noqa: F811
    assert not any(n.rstrip().endswith("::PieceRoot>") or "::PieceRoot>(" in n for n in kernels if "OpenPieceRoot" in n)


@pytest.mark.parametrize("name", OLDER_KERNELS + sorted(NEW_KERNELS))
def test_every_name_matches_exactly_one_kernel(kernels, name):      # noqa: F811
    """The budget tests find kernels by name after a word boundary and demand exactly one match."""
    assert len(_of(kernels, name)) == 1, name
