"""
The overlap table's two oracles against each other, and overlap_scores -- the host half of
compare_segmentations, which needs no GPU -- against a second writing of the same formulas
(tests/overlaps_ref.py), against scikit-learn, and against the identities the definitions imply. No GPU.

Tolerances. Integers and Fractions are compared exactly. Entropies to 1e-9 bits: the values have at most 31
bits, the tables at most about 1e4 rows, so the summation error is below 1e4 * 2.2e-16 * 31 < 1e-10.
"""

import math
from fractions import Fraction

import numpy as np
import pytest

import label_symmetry
import overlaps_ref
from aind_exaspim_neuron_segmentation_amd import segmentation
from aind_exaspim_neuron_segmentation_amd.segmentation import overlap_scores  # noqa: F401  (what this file is about)

SEEDS = list(range(40))
MODES = ("a", "both_zero", "none")
BITS = 1e-9
EXACT = ("n", "segments_a", "segments_b", "pairs", "same_partition")
RATIONAL = ("rand_precision", "rand_recall", "adapted_rand_error", "rand_index", "largest_overlap_agreement")
WHERE_THE_DENOMINATOR_IS_ZERO = {"rand_precision": 1.0, "rand_recall": 1.0, "adapted_rand_error": 0.0,
                                 "rand_index": 1.0, "largest_overlap_agreement": 1.0}


def assert_scores(got, want):
    assert sorted(got) == sorted(want)
    for key in EXACT:
        assert got[key] == want[key] and type(got[key]) is type(want[key]), key
    for key in RATIONAL:
        expected = WHERE_THE_DENOMINATOR_IS_ZERO[key] if want[key] is None else float(want[key])
        assert isinstance(got[key], float) and got[key] == expected, (key, got[key], want[key])
    for key in ("voi_split", "voi_merge", "voi"):
        assert isinstance(got[key], float) and abs(got[key] - want[key]) <= BITS, (key, got[key], want[key])
        assert got[key] >= 0.0


@pytest.mark.parametrize("seed", SEEDS)
def test_the_two_oracles_agree(seed):
    a, b = overlaps_ref.volumes(seed)
    pairs, counts = overlaps_ref.table_unique(a, b)
    pairs_b, counts_b = overlaps_ref.table_dict(a, b)
    assert pairs.dtype == pairs_b.dtype == np.int32 and counts.dtype == counts_b.dtype == np.int64
    np.testing.assert_array_equal(pairs, pairs_b)
    np.testing.assert_array_equal(counts, counts_b)
    assert int(counts.sum()) == a.size and pairs.min() >= 0
    assert len({tuple(r) for r in pairs.tolist()}) == len(pairs)


def test_the_seeded_volumes_hold_what_they_promise():
    seen = {"negative": 0, "min": 0, "max": 0, "sparse": 0, "ordered": 0}
    for seed in SEEDS:
        a, b = overlaps_ref.volumes(seed)
        seen["negative"] += bool(((a < 0) & (a > overlaps_ref.INT32_MIN)).any())
        seen["min"] += bool((b == overlaps_ref.INT32_MIN).any())
        seen["max"] += bool((a == overlaps_ref.INT32_MAX).any() or (b == overlaps_ref.INT32_MAX).any())
        seen["sparse"] += bool((a > 2048).any())
        rows = {tuple(r) for r in overlaps_ref.table_unique(a, b)[0].tolist()}
        seen["ordered"] += any((j, i) in rows for i, j in rows if i != j)
    assert all(v >= 3 for v in seen.values()), seen


@pytest.mark.parametrize("background", MODES)
@pytest.mark.parametrize("seed", SEEDS)
def test_scores_against_the_second_writing(seed, background):
    pairs, counts = overlaps_ref.table_unique(*overlaps_ref.volumes(seed))
    assert_scores(segmentation.overlap_scores(pairs, counts, background=background),
                  overlaps_ref.scores(pairs, counts, background))


def test_scores_on_a_large_table_with_counts_beyond_32_bits():
    """About 1e4 rows and sums of squares beyond 2^63: Python integers, no float before the last division."""
    rng = np.random.default_rng(7)
    keys = np.unique(rng.integers(0, 300, size=(12000, 2)), axis=0).astype(np.int32)
    counts = rng.integers(1, 2**40, size=len(keys)).astype(np.int64)
    assert len(keys) > 9000 and sum(int(c)**2 for c in counts) > 2**63
    for background in MODES:
        assert_scores(segmentation.overlap_scores(keys, counts, background=background),
                      overlaps_ref.scores(keys, counts, background))


@pytest.mark.parametrize("seed", SEEDS[:12])
def test_scores_against_scikit_learn(seed):
    cluster = pytest.importorskip("sklearn.metrics.cluster")
    a, b = overlaps_ref.volumes(seed)
    a, b = overlaps_ref.fold(a).ravel(), overlaps_ref.fold(b).ravel()
    got = segmentation.overlap_scores(*overlaps_ref.table_unique(a.astype(np.int32), b.astype(np.int32)),
                                      background="none")

    def entropy(v):
        p = np.unique(v, return_counts=True)[1] / v.size
        return float(-(p * np.log2(p)).sum())

    mutual = cluster.mutual_info_score(a, b) / math.log(2)
    assert abs(got["voi_split"] - (entropy(b) - mutual)) <= BITS
    assert abs(got["voi_merge"] - (entropy(a) - mutual)) <= BITS
    # pairs of voxels: [1, 1] together in both, [1, 0] together in a only, [0, 1] together in b only
    c = [[int(v) for v in row] for row in cluster.pair_confusion_matrix(a, b)]
    for key, denominator in (("rand_precision", c[1][1] + c[0][1]), ("rand_recall", c[1][1] + c[1][0])):
        assert got[key] == (float(Fraction(c[1][1], denominator)) if denominator else 1.0), key
    assert got["rand_index"] == (float(Fraction(c[0][0] + c[1][1], sum(map(sum, c)))) if a.size > 1 else 1.0)
    assert abs(got["rand_index"] - cluster.rand_score(a, b)) <= 1e-12 or a.size < 2


@pytest.mark.parametrize("seed", SEEDS)
def test_voi_is_zero_exactly_where_the_partitions_are_the_same(seed):
    a, b = overlaps_ref.volumes(seed)
    renamed = np.where(a > 0, (a.astype(np.int64) * 7 + 3) % 2147483629 + 1, a).astype(np.int32)      # injective
    for x, y, same in ((a, b, None), (a, renamed, True), (a, a, True)):
        pairs, counts = overlaps_ref.table_unique(x, y)
        for background in MODES:
            got = segmentation.overlap_scores(pairs, counts, background=background)
            assert (got["voi"] == 0.0) == got["same_partition"], (background, got)
            if same:
                assert got["same_partition"] and got["adapted_rand_error"] == 0.0 and got["rand_index"] == 1.0
                assert got["largest_overlap_agreement"] == 1.0


@pytest.mark.parametrize("seed", SEEDS)
def test_swapping_the_volumes_swaps_split_and_merge(seed):
    a, b = overlaps_ref.volumes(seed)
    ab = segmentation.overlap_scores(*overlaps_ref.table_unique(a, b), background="none")
    ba = segmentation.overlap_scores(*overlaps_ref.table_unique(b, a), background="none")
    for here, there in (("voi_split", "voi_merge"), ("rand_precision", "rand_recall"),
                        ("segments_a", "segments_b")):
        assert ab[here] == ba[there] and ab[there] == ba[here], here
    for key in ("n", "pairs", "adapted_rand_error", "rand_index", "same_partition"):
        assert ab[key] == ba[key], key
    assert abs(ab["voi"] - ba["voi"]) <= 1e-12


@pytest.mark.parametrize("seed", SEEDS[:10])
def test_renaming_the_labels_changes_no_score(seed):
    rng = np.random.default_rng(seed)
    shape = (5, 7, 23)
    a = overlaps_ref.blocky(rng, shape, 9, 6)
    b = np.where(rng.random(shape) < 0.85, a, overlaps_ref.blocky(rng, shape, 6, 9)).astype(np.int32)
    base = {m: segmentation.overlap_scores(*overlaps_ref.table_unique(a, b), background=m) for m in MODES}
    maps_a, maps_b = label_symmetry.label_maps(int(a.max()), seed), label_symmetry.label_maps(int(b.max()), seed + 1)
    assert sorted(maps_a) == ["one_home_slot", "permutation", "sparse"]
    for name in maps_a:
        ra, rb = label_symmetry.relabel_volume(a, maps_a[name]), label_symmetry.relabel_volume(b, maps_b[name])
        for mode in MODES:
            got = segmentation.overlap_scores(*overlaps_ref.table_unique(ra, rb), background=mode)
            for key, value in base[mode].items():
                if key.startswith("voi"):      # the rows are summed in another order
                    assert abs(got[key] - value) <= 1e-12, (name, mode, key)
                else:
                    assert got[key] == value, (name, mode, key)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_tools_old_agreement_rule(seed):
    a, b = overlaps_ref.volumes(seed)
    pairs, counts = overlaps_ref.table_unique(a, b)
    want = overlaps_ref.old_agreement(a, b)
    for background in MODES:
        assert segmentation.overlap_scores(pairs, counts, background=background)["largest_overlap_agreement"] == want


def test_the_empty_and_the_degenerate_tables():
    empty = segmentation.overlap_scores(np.zeros((0, 2), np.int32), np.zeros(0, np.int64), background="none")
    assert empty["n"] == 0 and empty["voi"] == 0.0 and empty["same_partition"] is True
    assert empty["rand_precision"] == empty["rand_recall"] == empty["rand_index"] == 1.0
    assert empty["adapted_rand_error"] == 0.0 and empty["largest_overlap_agreement"] == 1.0
    only_background = segmentation.overlap_scores(np.array([[0, 0]], np.int32), np.array([9]), background="a")
    assert only_background["n"] == 0 and only_background["pairs"] == 0
    singletons = segmentation.overlap_scores(np.array([[1, 1], [2, 2]], np.int32), np.array([1, 1]), background="a")
    assert singletons["rand_precision"] == singletons["rand_recall"] == 1.0 and singletons["adapted_rand_error"] == 0.0
    assert singletons["rand_index"] == 1.0 and singletons["same_partition"] is True


def test_overlap_scores_refuses():
    pairs, counts = np.array([[1, 1], [1, 2]], np.int32), np.array([3, 4], np.int64)
    with pytest.raises(ValueError, match="background"):
        segmentation.overlap_scores(pairs, counts, background="x")
    with pytest.raises(TypeError, match="integer"):
        segmentation.overlap_scores(pairs.astype(np.float32), counts)
    with pytest.raises(ValueError, match=r"\(P, 2\)"):
        segmentation.overlap_scores(pairs[:, :1], counts)
    with pytest.raises(ValueError, match="positive"):
        segmentation.overlap_scores(pairs, np.array([3, 0]))
    with pytest.raises(ValueError, match="more than one row"):
        segmentation.overlap_scores(np.array([[1, 1], [1, 1]], np.int32), counts)
