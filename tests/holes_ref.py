"""
CPU oracles of fill_holes (exaspim_fill_holes), written from the definition, and the volumes
the CPU and GPU tests share.

The definition: a voxel is background iff labels <= 0; a cavity is a 6-connected component of background
voxels; a cavity is a hole of label L iff none of its voxels lies on a face of the volume and the positive
labels among the six neighbours of its voxels are exactly the one value L; every voxel of a hole of L
becomes L and every other voxel keeps its value.

  by_components  the definition itself: scipy.ndimage.label of the background, per component the face test
                 and the set of positive labels among its voxels' 6-neighbours.
  per_label      the union over every L of scipy.ndimage.binary_fill_holes(labels == L) (scipy's default
                 6-connected structure), each written as L; it also reports whether any positive voxel
                 lies inside another label's filled region, where the two forms are not claimed to agree.
"""

import numpy as np
from scipy import ndimage

INT32_MAX = 2**31 - 1


def by_components(labels):
    """
    Returns
    -------
    out : numpy.ndarray
        int32, labels with every hole filled.
    stats : dict
        filled (cavities that are holes), voxels (voxels filled), open (cavities rejected for touching a
        face), mixed (closed cavities rejected for two or more neighbouring labels).
    """
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    assert labels.ndim == 3
    out = labels.copy()
    comp, n = ndimage.label(labels <= 0)      # the default structure is the 6-neighbourhood
    stats = dict(filled=0, voxels=0, open=0, mixed=0)
    if n == 0:
        return out, stats
    on_face = np.zeros(n + 1, dtype=bool)
    for axis in range(3):
        for index in (0, -1):
            on_face[np.unique(np.take(comp, index, axis=axis))] = True
    pairs = []      # (cavity, positive label next to one of its voxels)
    for axis in range(3):
        low = [slice(None)] * 3
        high = [slice(None)] * 3
        low[axis], high[axis] = slice(None, -1), slice(1, None)
        low, high = tuple(low), tuple(high)
        for here, there in ((low, high), (high, low)):
            c, l = comp[here], labels[there]
            sel = (c > 0) & (l > 0)
            pairs.append(np.stack([c[sel].astype(np.int64), l[sel].astype(np.int64)], axis=1))
    pairs = np.unique(np.concatenate(pairs, axis=0), axis=0)
    distinct = np.bincount(pairs[:, 0], minlength=n + 1)      # the size of each cavity's set of labels
    the_label = np.zeros(n + 1, dtype=np.int64)
    the_label[pairs[:, 0]] = pairs[:, 1]                      # meaningful where distinct == 1
    ids = np.arange(n + 1)
    hole = ~on_face & (distinct == 1) & (ids > 0)
    # a closed cavity has a positive neighbour: what bounds it is not background
    assert not (~on_face & (distinct == 0) & (ids > 0)).any()
    fill = hole[comp]
    out[fill] = the_label[comp[fill]].astype(np.int32)
    stats["filled"] = int(hole.sum())
    stats["voxels"] = int(fill.sum())
    stats["open"] = int(on_face[1:].sum())
    stats["mixed"] = int((~on_face & (distinct >= 2) & (ids > 0)).sum())
    return out, stats


def per_label(labels, on_label=None):
    """
    Every label is filled inside its own bounding box: a cavity that L encloses lies inside L's box, and a
    voxel of the complement on the box's border is either on a face of the volume or next to the outside of
    the box, which holds no L and reaches a face. on_label(rank, total), if given, is called before each
    label (a measurement aid: it may raise to stop).

    Returns
    -------
    out : numpy.ndarray
        int32: the union over every L of binary_fill_holes(labels == L), written as L over the background
        voxels it adds (in ascending order of L, the first writer stays).
    enclosed : bool
        Some positive voxel lies inside the filled region of another label.
    """
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    assert labels.ndim == 3
    out = labels.copy()
    enclosed = False
    written = np.zeros(labels.shape, dtype=bool)
    values = np.unique(labels[labels > 0])
    # find_objects wants small non-negative ids: the rank of each value
    ranks = np.searchsorted(values, np.where(labels > 0, labels, values[0] if values.size else 0)) + 1
    ranks[labels <= 0] = 0
    for rank, box in enumerate(ndimage.find_objects(ranks), start=1):
        if on_label is not None:
            on_label(rank, len(values))
        value = values[rank - 1]
        crop = labels[box]
        own = crop == value
        added = ndimage.binary_fill_holes(own) & ~own
        if (crop[added] > 0).any():
            enclosed = True
        new = added & (crop <= 0) & ~written[box]
        out[box][new] = value
        written[box] |= new
    return out, enclosed


# ---- the seeded volumes ---------------------------------------------------------------------------------
SEEDS = range(40)
DENSITIES = (0.05, 0.15, 0.3)


def blocky(rng, shape, top, block=4):
    """A field of labels 1 .. top that is constant on block^3 cells."""
    coarse = rng.integers(1, top + 1, size=tuple(-(-s // block) for s in shape))
    for axis in range(3):
        coarse = np.repeat(coarse, block, axis=axis)
    return np.ascontiguousarray(coarse[:shape[0], :shape[1], :shape[2]], dtype=np.int32)


def punched(rng, labels, density):
    """labels with a fraction "density" of its voxels set to background, half of them 0 and half -3."""
    out = labels.copy()
    punch = rng.random(labels.shape) < density
    value = np.where(rng.random(labels.shape) < 0.5, 0, -3).astype(np.int32)
    out[punch] = value[punch]
    return out


def seeded_volume(seed):
    """Sides 3 .. 14, a 4^3-blocky field of 1 .. 3 labels, punched at density 0.05, 0.15 or 0.3."""
    rng = np.random.default_rng(4000 + seed)
    shape = tuple(int(v) for v in rng.integers(3, 15, size=3))
    top = int(rng.integers(1, 4))
    return punched(rng, blocky(rng, shape, top), DENSITIES[seed % 3])


# ---- the hand-built cases: (name, labels, expected by construction) -------------------------------------
def _solid(shape, value):
    return np.full(shape, value, dtype=np.int32)


def hand_cases():
    cases = []

    def add(name, labels, want):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        want = np.ascontiguousarray(want, dtype=np.int32)
        labels.setflags(write=False)
        want.setflags(write=False)
        cases.append((name, labels, want))

    a = _solid((5, 5, 5), 7)
    a[2, 2, 2] = 0
    add("one_voxel_hole", a, _solid((5, 5, 5), 7))

    a = _solid((5, 5, 5), 7)
    a[1, 2, 2] = 0
    add("one_voxel_from_a_face", a, _solid((5, 5, 5), 7))

    # a 2 x 2 x 2 cavity with one more voxel on one of its corner voxels, and that one lies on the face z = 0
    a = _solid((6, 6, 6), 4)
    a[1:3, 1:3, 1:3] = 0
    a[0, 1, 1] = 0
    add("touches_a_face_at_one_corner_voxel", a, a)

    # (2, 2, 2) and (2, 3, 3) share an edge and no face: two cavities; the second one also has M = 3 next to it
    # (a row of M that reaches the face x = 5, so that M is not itself enclosed by L)
    a = _solid((6, 6, 6), 2)
    a[2, 2, 2] = 0
    a[2, 3, 3] = 0
    a[2, 3, 4:] = 3
    want = a.copy()
    want[2, 2, 2] = 2
    add("two_cavities_meeting_along_an_edge", a, want)

    a = _solid((7, 7, 7), 5)
    a[2:5, 2:5, 2:5] = 0
    a[3, 3, 3] = 9
    add("island_of_another_label", a, a)

    a = _solid((7, 7, 7), 5)
    a[2:5, 2:5, 2:5] = 0
    a[3, 3, 3] = 5
    add("floating_piece_of_the_same_label", a, _solid((7, 7, 7), 5))

    a = _solid((5, 6, 7), 3)
    a[2, 2:4, 2:5] = 0
    a[2, 2, 3] = -3
    a[2, 3, 4] = -(2**31)
    a[2, 3, 2] = -1
    add("negative_voxels_inside_a_hole", a, _solid((5, 6, 7), 3))

    a = _solid((5, 5, 5), INT32_MAX)
    a[2, 2, 2] = 0
    a[2, 2, 3] = -5
    add("label_int32_max", a, _solid((5, 5, 5), INT32_MAX))

    for axis in range(3):
        shape = [5, 5, 5]
        shape[axis] = 1
        a = _solid(tuple(shape), 6)
        a[tuple(0 if i == axis else 2 for i in range(3))] = 0
        add(f"single_voxel_axis_{axis}", a, a)

    add("one_voxel_background", np.zeros((1, 1, 1)), np.zeros((1, 1, 1)))
    add("one_voxel_label", _solid((1, 1, 1), 4), _solid((1, 1, 1), 4))

    a = np.zeros((4, 5, 6), dtype=np.int32)
    a[1, 2, 3] = -3
    a[2, 2, 2] = -(2**31)
    add("all_background", a, a)

    add("all_one_label", _solid((4, 5, 6), 8), _solid((4, 5, 6), 8))
    return cases


def carve(labels, points, value=0):
    """Sets the voxels of the axis-aligned polyline through "points" to value (a one-voxel-wide snake)."""
    for p, q in zip(points, points[1:]):
        assert sum(a != b for a, b in zip(p, q)) <= 1, (p, q)
        index = tuple(slice(min(a, b), max(a, b) + 1) for a, b in zip(p, q))
        labels[index] = value
    return labels
