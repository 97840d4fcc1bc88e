"""
The float64 oracle of stage 6 of skeletonize_labels, the one device computation of the label chain
that is torch arithmetic and no kernel of the project's:

    cost[v] = pdrf_scale * (1 - sqrt(dbf[v]) / sqrt(peak[L])) ** pdrf_exponent + daf[v] / far[L],   L = labels[v]

peak[L] is the largest dbf of label L, far[L] the largest finite daf of L; either term is 0 where its divisor is
0, and 0 ** 0 is 1. It is defined on the voxels with 1 <= labels <= k; background voxels are not compared. Where
daf is +inf (a piece of a label that the root's piece does not touch) and far > 0 the cost is +inf.

cost() is written on whole arrays, by_label() label by label in code of its own; the volumes are the ones the
CPU and GPU tests share.
"""

import numpy as np

DBF_INF = 2**31 - 1
EPS = 2.0 ** -24      # half an ulp of 1 in float32: the relative error of one rounded operation


def bound(pdrf_exponent, pdrf_scale):
    """
    The absolute error allowed to a float32 evaluation: (4 e + 16) * 2^-24 * (pdrf_scale + 1). Derived, not
    fitted: two conversions / square roots and one division give the quotient q <= 1 with 3 rounded operations,
    1 - q is one more (absolute error <= 4 * 2^-24 on a value <= 1), the power amplifies that e times and adds
    its own rounding, the product with pdrf_scale, the division daf / far and the sum are one rounding each on
    values <= pdrf_scale, 1 and pdrf_scale + 1; the constant 16 covers those and a pow that is a few ulp off.
    """
    return (4 * pdrf_exponent + 16) * EPS * (float(pdrf_scale) + 1.0)


def inside_of(labels, k):
    labels = np.asarray(labels)
    return (labels >= 1) & (labels <= k)


def maxima(labels, dbf, daf, k):
    """(peak int64 (k + 1,), far float64 (k + 1,)): per label the largest dbf and the largest finite daf, 0 for
    an absent label, for a label without a finite daf and in row 0."""
    labels, dbf, daf = np.asarray(labels), np.asarray(dbf), np.asarray(daf)
    inside = inside_of(labels, k)
    peak = np.zeros(k + 1, dtype=np.int64)
    np.maximum.at(peak, labels[inside], dbf[inside].astype(np.int64))
    far = np.zeros(k + 1, dtype=np.float64)
    finite = inside & np.isfinite(daf)
    np.maximum.at(far, labels[finite], daf[finite].astype(np.float64))
    return peak, far


def cost(labels, dbf, daf, k, pdrf_exponent, pdrf_scale):
    """float64 array of the labels' shape; NaN on the voxels that are not compared (labels outside 1..k)."""
    labels = np.asarray(labels)
    inside = inside_of(labels, k)
    rows = np.where(inside, labels, 0)
    peak, far = maxima(labels, dbf, daf, k)
    peak_v, far_v = peak[rows].astype(np.float64), far[rows]
    d = np.asarray(dbf).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(peak_v > 0, 1.0 - np.sqrt(np.maximum(d, 0.0)) / np.sqrt(peak_v), 0.0)
        first = np.where(peak_v > 0, np.float64(pdrf_scale) * np.power(depth, np.float64(pdrf_exponent)), 0.0)
        second = np.where(far_v > 0, np.asarray(daf).astype(np.float64) / far_v, 0.0)
    return np.where(inside, first + second, np.nan)


def by_label(labels, dbf, daf, k, pdrf_exponent, pdrf_scale):
    """The same definition, one label at a time and one voxel at a time, in Python floats (math, not numpy)."""
    import math

    labels = np.asarray(labels)
    flat_l, flat_d, flat_a = labels.reshape(-1), np.asarray(dbf).reshape(-1), np.asarray(daf).reshape(-1)
    out = np.full(labels.size, np.nan, dtype=np.float64)
    for row in range(1, k + 1):
        mine = np.flatnonzero(flat_l == row)
        if mine.size == 0:
            continue
        peak = max(int(flat_d[v]) for v in mine)
        finite = [float(flat_a[v]) for v in mine if math.isfinite(float(flat_a[v]))]
        far = max(finite) if finite else 0.0
        for v in mine:
            first = 0.0
            if peak > 0:
                depth = 1.0 - math.sqrt(max(int(flat_d[v]), 0)) / math.sqrt(peak)
                first = float(pdrf_scale) * (1.0 if pdrf_exponent == 0 else depth ** int(pdrf_exponent))
            second = float(flat_a[v]) / far if far > 0 else 0.0
            out[v] = first + second
    return out.reshape(labels.shape)


def worst_ratio(got, want, labels, k, pdrf_exponent, pdrf_scale):
    """
    max |got - want| / bound over the compared voxels with a finite reference, after the checks that need no
    tolerance: no compared voxel is NaN, and got is +inf exactly where the reference is.
    """
    got, want = np.asarray(got), np.asarray(want)
    inside = inside_of(labels, k)
    assert not np.isnan(got[inside]).any(), "a compared voxel is NaN"
    assert not np.isnan(want[inside]).any()
    infinite = inside & np.isinf(want)
    assert (got[infinite] == np.inf).all(), "the reference is +inf where the field is not"
    finite = inside & ~infinite
    assert np.isfinite(got[finite]).all(), "the field is not finite where the reference is"
    if not finite.any():
        return 0.0
    return float(np.abs(got[finite].astype(np.float64) - want[finite]).max() / bound(pdrf_exponent, pdrf_scale))


# ---- volumes -------------------------------------------------------------------------------------------------
def chain_volume():
    """(a) the volume of test_skeletonize_labels_against_the_oracles: blocky labels and a bar with a cavity."""
    import holes_ref

    labels = np.ascontiguousarray(holes_ref.seeded_volume(7), dtype=np.int32)
    big = np.zeros((16, 20, 40), dtype=np.int32)
    big[1:1 + labels.shape[0], 2:2 + labels.shape[1], 3:3 + labels.shape[2]] = labels
    big[10:15, 14:19, 20:38] = 5
    big[12, 16, 25:28] = 0
    return big


def absent_ids():
    """(b) ids 1, 3 and 6 present, 2, 4 and 5 absent: table rows with peak = 0 and far = 0 are gathered from."""
    v = np.zeros((8, 12, 40), dtype=np.int32)
    v[1:6, 1:7, 2:20] = 1
    v[3, 3, 5:9] = 0          # a cavity: filled
    v[2:7, 7:11, 22:38] = 3
    v[0:3, 8:12, 0:12] = 6
    v[6:8, 0:5, 30:40] = 6    # a second piece of 6
    return v


def dots_and_a_line():
    """(c) one-voxel labels (far = 0, dbf = peak) and a one-voxel-thick line of 70 voxels along x that crosses
    the tile seams at x = 32 and x = 64."""
    v = np.zeros((4, 6, 80), dtype=np.int32)
    v[1, 1, 3] = 1
    v[2, 4, 5:75] = 2
    v[3, 5, 79] = 3           # in the volume's last corner
    v[0, 0, 0] = 4            # and in its first
    return v


def pieces():
    """(d) label 1 in two pieces that do not touch; label 2 in two blocks that touch only at a corner (one piece
    for the 26-neighbourhood of the fields)."""
    v = np.zeros((10, 12, 40), dtype=np.int32)
    v[1:4, 1:5, 1:12] = 1
    v[6:9, 7:11, 25:38] = 1
    v[1:4, 6:9, 16:20] = 2
    v[4:7, 9:12, 20:24] = 2   # shares only the corner (4, 9, 20) | (3, 8, 19)
    return v


def solid():
    """(e) one label that fills the volume: dbf is DBF_INF everywhere, the first term is 0 everywhere."""
    return np.ones((6, 9, 40), dtype=np.int32)


def one_plane():
    """(f) a (1, 24, 40) volume."""
    rng = np.random.default_rng(606)
    v = np.zeros((1, 24, 40), dtype=np.int32)
    v[0, 2:11, 3:37] = 1
    v[0, 13:22, 1:18] = 2
    v[0, 12:23, 20:39] = 3
    v[0][(rng.random((24, 40)) < 0.12)] = 0
    v[0, 6, 3:37] = 1         # a spine through label 1
    return v


VOLUMES = {"a": chain_volume, "b": absent_ids, "c": dots_and_a_line, "d": pieces, "e": solid, "f": one_plane}
