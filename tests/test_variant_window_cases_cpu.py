"""The two cases test_gpu_variant_window.py runs on every network variant, planned on the host with each variant's
host model (carry_ref.py with the variant's padded level widths): they must keep the traits that make them worth
running there -- links, a cut chain, second-level ranges exactly for the variants that have a second level, and
nothing at all for the variant without row mode -- and the host model's buffer sizes must be the real model's."""

import pytest

import variant_models as V
import window_fuzz_cases as W
from carry_ref import _Model, _RowModel

CASES = V.window_cases()
SMALLEST, CUT = CASES["smallest"], CASES["cut"]


def test_the_cases_are_the_ones_described():
    assert (SMALLEST["shape"], SMALLEST["patch"]) == ((64, 24, 96), (32, 16, 64))
    assert (CUT["shape"], CUT["patch"], CUT["overlap"][0]) == ((112, 56, 96), (48, 32, 64), 32)
    # the seeds test_gpu_window_fuzz.py runs the same cases with
    by_id = {W.case_id(c): c for c in W.cases()}
    assert by_id[W.case_id(SMALLEST)] == SMALLEST and by_id[W.case_id(CUT)] == CUT


def test_the_defaults_are_the_full_width_model():
    for cls in (_Model, _RowModel):
        m = cls()
        assert (m.c0p, m.c1p) == (32, 64)
        assert m.carry_pair_elems((2, 48, 16, 64)) == (2 * 48 * 16 * 64 * 32, 2 * 48 * 16 * 64 * 4)
        assert m.carry_triple_elems((2, 48, 16, 64)) == (2 * 48 * 16 * 64 * 8, 2 * 48 * 16 * 64 * 8, 2 * 48 * 16 * 64)


@pytest.mark.parametrize("name", V.NAMES)
def test_padded_widths_and_buffer_sizes_are_the_models(name):
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    v = V.VARIANTS[name]
    model = UNet3D(output_channels=v["out"], trilinear=v["trilinear"], width_multiplier=v["wm"])
    host = V.host_model(name)
    assert (host.c0p, host.c1p) == {"foreground": (32, 64), "convt": (32, 64), "three_quarter": (32, 64),
                                    "half": (32, 32), "double": (64, 128)}[name]
    # row mode iff level 0 is no whole 64-cout slice, a second level iff level 1 is whole 64-cout slices and
    # there is a first
    assert v["row"] == (host.c0p % 64 != 0)
    assert v["level1"] == (v["row"] and host.c1p % 64 == 0)
    for shape in ((2, 48, 16, 64), (2, 32, 16, 64), (3, 48, 32, 64)):
        assert host.carry_pair_elems(shape) == model.carry_pair_elems(shape)
        assert host.carry_triple_elems(shape) == model.carry_triple_elems(shape)
    # the C ABI geometry of test_gpu_variant_plans.py
    span = host.carry_planes((2, 48, 16, 64), 32, 16)
    assert (span[1] > span[0]) == v["row"] and span == ((6, 30) if v["row"] else (0, 0))
    assert host.carry1_planes((2, 48, 16, 64), 32, 16) == ((4, 12) if v["level1"] else (0, 0))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", V.NAMES)
def test_the_cases_keep_their_traits_on_every_variant(name, case):
    v = V.VARIANTS[name]
    host = V.host_model(name)
    t = W.traits(CASES[case], host)
    p = W.plan(CASES[case], host)
    print(name, case, t)
    if not v["row"]:
        assert t["links"] == 0 and t["cuts"] == 0 and t["level1"] == 0 and t["rows"] == 0
        assert p["links"] == [None] * t["batches"] and (p["peak"], p["level1"]) == (0, False)
        return
    assert t["links"] >= 1 and t["rows"] == t["batches"]
    if case == "cut":
        assert t["cuts"] >= 1
        # a second-level range exactly for the variants that have a second level
        assert (t["level1"] >= 1) == v["level1"] and p["level1"] == v["level1"]
    else:       # 32 deep: no whole level-1 tile from plane 4 on, whatever the variant
        assert t["level1"] == 0 and not p["level1"]
    # the first level's links do not depend on the second level's width
    base = W.plan(CASES[case])
    assert [l and l[:3] for l in p["links"]] == [l and l[:3] for l in base["links"]] and p["peak"] == base["peak"]
    if not v["level1"]:
        assert all(l is None or l[3] == (0, 0) for l in p["links"])
    else:
        assert p["links"] == base["links"]


def test_a_second_level_range_is_reached_where_there_is_a_second_level():
    """Of the two cases at least one link with a second-level range for the three variants with a second level,
    none for the others."""
    for name in V.NAMES:
        n = sum(W.traits(c, V.host_model(name))["level1"] for c in CASES.values())
        assert (n >= 1) == V.VARIANTS[name]["level1"], (name, n)
