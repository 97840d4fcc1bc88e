"""
Host oracles for border_targets (no GPU), written from the definition in include/exaspim_affinity.h
(DESIGN 6p): the six faces of a labelled volume, per face the 8-connected components of every label in 1..K, per
component the pixel with the largest e -- the least squared in-plane distance to a pixel of another label or to a
position just outside the plane -- ties to the smallest linear voxel index.

(A) brute_force: e per plane by the minimum over every other-labelled pixel and every position of a one-pixel ring
    around the plane (a farther outside position is never nearer than the ring's).
(B) by_component: per component, scipy's exact Euclidean distance transform of the component's mask padded by one
    pixel of background, squared and rounded: the distance to "not this component". DESIGN 6p proves that the two
    are the same; tests/test_border_ref_cpu.py holds them to each other.

Both return the sorted, deduplicated list of (label, voxel index) as an int64 (T, 2) array.
"""

import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), dtype=bool)

SHAPES = [(1, 5, 5), (2, 2, 2), (5, 1, 130), (3, 66, 65), (7, 9, 70), (65, 3, 63), (4, 8, 8), (1, 1, 63), (1, 1, 64)]


def faces(labels):
    """The six (plane of labels, plane of linear voxel indices), in the order z0, z1, y0, y1, x0, x1."""
    labels = np.asarray(labels)
    index = np.arange(labels.size, dtype=np.int64).reshape(labels.shape)
    cuts = [(0, 0), (0, -1), (1, 0), (1, -1), (2, 0), (2, -1)]
    return [(np.take(labels, at, axis=axis), np.take(index, at, axis=axis)) for axis, at in cuts]


def foreground(plane, k):
    return np.where((plane >= 1) & (plane <= k), plane, 0).astype(np.int64)


def e_brute_force(plane):
    """e of every foreground pixel of a plane whose background is 0; 0 on the background."""
    h, w = plane.shape
    ring = np.full((h + 2, w + 2), -1, dtype=np.int64)
    ring[1:-1, 1:-1] = plane
    rows, cols = np.indices(ring.shape)
    out = np.zeros((h, w), dtype=np.int64)
    for value in np.unique(plane[plane > 0]):
        mine = np.argwhere(plane == value)
        other = ring != value
        oy, ox = rows[other] - 1, cols[other] - 1
        for start in range(0, len(mine), 256):
            part = mine[start:start + 256]
            d2 = (part[:, 0, None] - oy[None, :]) ** 2 + (part[:, 1, None] - ox[None, :]) ** 2
            out[part[:, 0], part[:, 1]] = d2.min(axis=1)
    return out


def e_by_component(mask):
    """The squared distance of every pixel of one component's mask to a pixel outside it or outside the plane."""
    padded = np.pad(mask, 1)
    return np.rint(ndimage.distance_transform_edt(padded)[1:-1, 1:-1] ** 2).astype(np.int64)


def _plane_targets(plane, index, per_plane_e):
    """(label, voxel index) of every component of one plane whose background is 0."""
    found = set()
    e_plane = per_plane_e(plane) if per_plane_e is not None else None
    for value in np.unique(plane[plane > 0]):
        components, _ = ndimage.label(plane == value, structure=EIGHT)
        for c, box in enumerate(ndimage.find_objects(components), start=1):
            mask = components[box] == c      # the component's bounding box: nothing of it lies outside
            e = e_plane[box] if e_plane is not None else e_by_component(np.pad(mask, 1))[1:-1, 1:-1]
            best = e[mask].max()
            found.add((int(value), int(index[box][mask & (e == best)].min())))
    return found


def _targets(labels, k, per_plane_e):
    found = set()
    for plane, index in faces(labels):
        found |= _plane_targets(foreground(plane, k), index, per_plane_e)
    return np.array(sorted(found), dtype=np.int64).reshape(-1, 2)


def brute_force(labels, k):
    """Oracle (A)."""
    return _targets(labels, k, e_brute_force)


def by_component(labels, k):
    """Oracle (B)."""
    return _targets(labels, k, None)


def face_targets(labels, k, face):
    """The targets of one face alone (0..5 in the order of faces()), as a sorted list of (label, voxel index)."""
    plane, index = faces(labels)[face]
    return sorted(_plane_targets(foreground(plane, k), index, None))


def random_volume(seed, shape, k=5, fill=0.6):
    """Seeded labels in 0..k: even seeds voxel noise, odd seeds blocks of 3 voxels so that components go deep."""
    rng = np.random.default_rng(seed)
    if seed % 2:
        coarse = tuple(-(-s // 3) for s in shape)
        values = np.where(rng.random(coarse) < fill, rng.integers(1, k + 1, size=coarse), 0)
        values = np.kron(values, np.ones((3, 3, 3), dtype=np.int64))[:shape[0], :shape[1], :shape[2]]
    else:
        values = np.where(rng.random(shape) < fill, rng.integers(1, k + 1, size=shape), 0)
    return np.ascontiguousarray(values, dtype=np.int32)


def _on_top(plane, depth=3):
    """A volume whose face z = 0 is the plane and whose other voxels are 0."""
    volume = np.zeros((depth,) + plane.shape, dtype=np.int32)
    volume[0] = plane
    return volume


def crafted():
    """name -> (labels, K, the number of targets on the face z = 0 or None)."""
    cases = {}
    plane = np.zeros((6, 7), dtype=np.int32)
    plane[1, 1] = plane[2, 2] = plane[3, 3] = plane[2, 4] = 1
    cases["joined only diagonally"] = (_on_top(plane), 1, 1)
    plane = np.zeros((9, 12), dtype=np.int32)
    plane[1:4, 1:4] = 1
    plane[5:8, 6:11] = 1
    cases["two components of one label"] = (_on_top(plane), 1, 2)
    plane = np.zeros((9, 11), dtype=np.int32)
    plane[1:3, 1:10] = 2
    plane[6:8, 1:10] = 2
    plane[1:8, 1:3] = 2      # a U on its side: columns 3..9 hold two runs of the one component
    cases["a U whose columns hold two runs"] = (_on_top(plane), 2, 1)
    checker = (np.indices((2, 7, 9)).sum(axis=0) % 2 + 1).astype(np.int32)
    cases["a two-label checkerboard"] = (checker, 2, 2)
    plane = np.zeros((7, 12), dtype=np.int32)
    plane[2:4, 1:10] = 3
    cases["a 2-wide bar"] = (_on_top(plane), 3, 1)
    y, x = np.indices((11, 13))
    plane = (((y - 5) ** 2 + (x - 6) ** 2) <= 10).astype(np.int32) * 4
    cases["a blob with a unique maximum"] = (_on_top(plane), 4, 1)
    volume = np.zeros((4, 5, 6), dtype=np.int32)
    volume[0, 0, 0] = 1      # a corner: three faces, one row
    volume[0, 0, 3] = 2      # an edge: two faces, one row
    volume[3, 2, 5] = 3      # a face and an edge of another pair
    cases["an edge and a corner"] = (volume, 3, None)
    volume = np.zeros((3, 5, 6), dtype=np.int32)
    volume[0, 1:3, 1:3] = 7
    volume[0, 3, 4] = -3
    volume[2, 1:4, 1:4] = 2
    volume[1, 0, 2:5] = 3
    cases["labels <= 0 and > K ignored"] = (volume, 2, 0)
    cases["an empty volume"] = (np.zeros((3, 4, 5), dtype=np.int32), 3, 0)
    return cases
