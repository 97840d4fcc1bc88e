"""
The kernels that exaspim_watershed_stream_slab adds, in the code-object metadata of the in-tree library (no GPU
needed, in the manner of test_kernel_budget_blocks.py): the slab's mask kernel is there for float32 and float16
and both vector widths, built for gfx950 wave64 and bound at 256 threads, uses neither scratch memory nor spills,
holds the LDS of edge_mask_watershed (read from the same metadata, not written down here) and stays within 64
registers, so that 8 waves per SIMD remain (DESIGN 6s writes the built counts next to that bound); the kernel that
carries the plane of z affinities is there for both types; and the new names hide no kernel that was there before.
"""

import re

import pytest

from test_kernel_budget import kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)

MASK = "edge_mask_watershed_slab"
SIBLING = "edge_mask_watershed"
INSTANCES = [("float", 4), ("float", 1), ("_Float16", 8), ("_Float16", 1)]
VGPR_BOUND = 64
OLDER_KERNELS = ["tile_pass", "face_merge", "flatten", "sizes", "relabel", "survey_faces", "survey", "fill",
                 "seam_mark", "seam_union", "slab_advance", "border_union", "border_gather", "table_flatten",
                 "table_sum", "table_spread", "pieces_tile_pass", "pieces_seam_merge", "pieces_sizes",
                 "pieces_relabel", "pieces_mark_open",
                 "scan_count<exaspim::(anonymous namespace)::PieceRoot>",
                 "scan_assign<exaspim::(anonymous namespace)::PieceRoot>",
                 "scan_count<exaspim::(anonymous namespace)::OpenPieceRoot>",
                 "scan_assign<exaspim::(anonymous namespace)::OpenPieceRoot>",
                 "scan_count<exaspim::(anonymous namespace)::SlabRoot>",
                 "scan_assign<exaspim::(anonymous namespace)::SlabRoot>"]


def _of(kernels, name):      # noqa: F811
    out = {n: k for n, k in kernels.items() if re.search(r"\b" + re.escape(name) + r"\(", n) and "exaspim::" in n}
    assert out, name
    return out


MANGLED = {"float": "f", "_Float16": "DF16_"}


def _instance(kernels, name, dtype, vec=None):      # noqa: F811
    """The instantiation name<dtype[, vec]>, by its demangled name or, where the demangler at hand does not know
    _Float16 and leaves the name as it is, by its mangled one."""
    plain = f"{name}<{dtype}" + (f", {vec}>" if vec is not None else ">")
    mangled = f"{len(name)}{name}I{MANGLED[dtype]}" + (f"Li{vec}E" if vec is not None else "") + "E"
    out = {n: k for n, k in kernels.items()
           if (re.search(r"\b" + re.escape(plain) + r"\(", n) and "exaspim::" in n)
           or (n.startswith("_ZN7exaspim") and "N_1" + mangled in n)}      # (anonymous namespace)::
    assert out, plain
    return out


@pytest.mark.parametrize("dtype,vec", INSTANCES)
def test_the_mask_kernel_is_there_once_per_type_and_width(kernels, dtype, vec):      # noqa: F811
    assert len(_instance(kernels, MASK, dtype, vec)) == 1
    assert len(_instance(kernels, SIBLING, dtype, vec)) == 1      # and its name has not hidden the sibling


@pytest.mark.parametrize("dtype,vec", INSTANCES)
def test_wave64_256_threads_no_scratch_no_spills(kernels, dtype, vec):      # noqa: F811
    (full, k), = _instance(kernels, MASK, dtype, vec).items()
    assert k[".wavefront_size"] == 64, full
    assert k[".max_flat_workgroup_size"] == 256, full
    assert k[".private_segment_fixed_size"] == 0, full
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full


@pytest.mark.parametrize("dtype,vec", INSTANCES)
def test_lds_is_the_siblings_and_eight_waves_per_simd_remain(kernels, dtype, vec):      # noqa: F811
    (full, k), = _instance(kernels, MASK, dtype, vec).items()
    (_, sibling), = _instance(kernels, SIBLING, dtype, vec).items()
    assert k[".group_segment_fixed_size"] == sibling[".group_segment_fixed_size"] > 0, full
    print(full, "vgprs", k[".vgpr_count"], "sibling", sibling[".vgpr_count"])
    assert k[".vgpr_count"] <= VGPR_BOUND, (full, k[".vgpr_count"])


@pytest.mark.parametrize("dtype", ["float", "_Float16"])
def test_the_carry_kernel(kernels, dtype):      # noqa: F811
    (full, k), = _instance(kernels, "seam_affinity", dtype).items()
    assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 256, full
    assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, full
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, full
    assert k[".vgpr_count"] <= 32, (full, k[".vgpr_count"])


@pytest.mark.parametrize("name", OLDER_KERNELS)
def test_every_older_name_still_matches_exactly_one_kernel(kernels, name):      # noqa: F811
    """The budget tests find kernels by name after a word boundary and demand exactly one match."""
    assert len(_of(kernels, name)) == 1, name
