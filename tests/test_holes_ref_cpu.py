"""
The two CPU oracles of fill_holes (tests/holes_ref.py) held to each other and to hand-built cases, without a
GPU: by_components is the definition (components of the background, the face test, the set of neighbouring
labels), per_label the union of scipy's binary_fill_holes over every label. They must agree on every
seeded volume where per_label reports no label enclosed by another, and the set of volumes must exercise
all three outcomes of a cavity.
"""

import numpy as np
import pytest

import holes_ref

CASES = holes_ref.hand_cases()


def test_the_two_oracles_agree_on_the_seeded_volumes():
    free, totals = 0, dict(filled=0, voxels=0, open=0, mixed=0)
    for seed in holes_ref.SEEDS:
        labels = holes_ref.seeded_volume(seed)
        assert labels.dtype == np.int32 and 3 <= min(labels.shape) and max(labels.shape) <= 14
        before = labels.copy()
        want, stats = holes_ref.by_components(labels)
        other, enclosed = holes_ref.per_label(labels)
        np.testing.assert_array_equal(labels, before)      # neither oracle writes into its argument
        for key in totals:
            totals[key] += stats[key]
        assert stats["voxels"] == int((want != labels).sum())
        assert (want[labels > 0] == labels[labels > 0]).all()      # positive voxels never change
        if not enclosed:
            free += 1
            np.testing.assert_array_equal(want, other, err_msg=f"seed {seed}")
    print(f"{len(holes_ref.SEEDS)} volumes, {free} without an enclosed label, cavities: {totals}")
    assert len(holes_ref.SEEDS) >= 40 and free >= 30
    assert totals["filled"] >= 100 and totals["open"] >= 100 and totals["mixed"] >= 100, totals


@pytest.mark.parametrize("name,labels,want", CASES, ids=[c[0] for c in CASES])
def test_hand_built_case(name, labels, want):
    got, stats = holes_ref.by_components(labels)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    assert stats["voxels"] == int((want != labels).sum())
    other, enclosed = holes_ref.per_label(labels)
    assert enclosed == (name == "island_of_another_label")
    if not enclosed:
        np.testing.assert_array_equal(other, want)


def test_what_the_hand_built_cases_cover():
    by_name = {name: (labels, want) for name, labels, want in CASES}
    filled = {n for n, (a, b) in by_name.items() if not np.array_equal(a, b)}
    assert filled == {"one_voxel_hole", "one_voxel_from_a_face", "two_cavities_meeting_along_an_edge",
                      "floating_piece_of_the_same_label", "negative_voxels_inside_a_hole", "label_int32_max"}
    labels, want = by_name["two_cavities_meeting_along_an_edge"]
    assert labels[2, 2, 2] == 0 and want[2, 2, 2] == 2 and labels[2, 3, 3] == 0 and want[2, 3, 3] == 0
    labels, want = by_name["island_of_another_label"]
    assert want[3, 3, 3] == 9 and (want[2:5, 2:5, 2:5] <= 0).sum() == 26
    labels, want = by_name["negative_voxels_inside_a_hole"]
    assert (labels < 0).sum() == 3 and (want == 3).all()
    labels, want = by_name["label_int32_max"]
    assert (want == 2**31 - 1).all()
    labels, _ = by_name["touches_a_face_at_one_corner_voxel"]
    on_face = np.zeros(labels.shape, dtype=bool)
    for axis in range(3):
        for index in (0, -1):
            on_face[tuple(index if i == axis else slice(None) for i in range(3))] = True
    assert ((labels == 0) & on_face).sum() == 1 and (labels == 0).sum() == 9
    for axis in range(3):
        assert by_name[f"single_voxel_axis_{axis}"][0].shape[axis] == 1
    stats = [holes_ref.by_components(by_name[n][0])[1] for n in ("one_voxel_hole", "island_of_another_label",
                                                                  "touches_a_face_at_one_corner_voxel")]
    assert [(s["filled"], s["open"], s["mixed"]) for s in stats] == [(1, 0, 0), (0, 0, 1), (0, 1, 0)]


def test_the_snake_helper():
    block = np.full((6, 6, 12), 2, dtype=np.int32)
    holes_ref.carve(block, [(2, 2, 2), (2, 2, 9), (2, 4, 9), (4, 4, 9)])
    assert (block == 0).sum() == 8 + 2 + 2
    got, stats = holes_ref.by_components(block)
    assert (got == 2).all() and stats == dict(filled=1, voxels=12, open=0, mixed=0)
    holes_ref.carve(block, [(4, 4, 9), (5, 4, 9)])      # one end reaches the face z = 5
    got, stats = holes_ref.by_components(block)
    np.testing.assert_array_equal(got, block)
    assert stats == dict(filled=0, voxels=0, open=1, mixed=0)
