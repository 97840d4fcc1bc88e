"""
CPU oracle of exaspim_components (include/exaspim_affinity.h): connected components of the
graph of "on" edges with scipy.sparse.csgraph, the reference's size filter
(img_util.py:555-558, kept iff size > min_size) and numbering 1 .. K in the order of each
component's smallest C-order linear index.

    components(aff, threshold, min_size) -> (labels int32 (D, H, W), K)

aff is (3, D, H, W) affinities (channel c at voxel v = edge v -- v + e_c, e = z, y, x; the last
index along axis c is ignored; a voxel without an on edge is background) or a (D, H, W)
foreground map (voxels >= threshold are on and 6-connected; a lone on voxel is a component of
size 1). float16 input is widened exactly; the threshold is rounded to float32; NaN is off.

affinities_of_foreground and drop_singletons derive an affinity-mode case and its labels from a foreground
and scipy.ndimage.label, for volumes where components() itself is too slow; tests/test_components_cpu.py
holds the two to components().
"""

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def edge_masks(aff, threshold):
    """(on_z, on_y, on_x, voxel_on): boolean (D, H, W) arrays; edge c of voxel v joins v and v + e_c."""
    thr = np.float32(threshold)
    aff = np.asarray(aff)
    if aff.dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(aff.dtype)
    a = aff.astype(np.float32)
    if a.ndim == 4:
        assert a.shape[0] == 3
        with np.errstate(invalid="ignore"):
            on = [a[c] >= thr for c in range(3)]
        voxel_on = None
    elif a.ndim == 3:
        with np.errstate(invalid="ignore"):
            voxel_on = a >= thr
        on = []
        for axis in range(3):
            e = np.zeros(a.shape, bool)
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            e[tuple(lo)] = voxel_on[tuple(lo)] & voxel_on[tuple(hi)]
            on.append(e)
    else:
        raise ValueError(a.ndim)
    for axis in range(3):   # entries that leave the volume
        last = [slice(None)] * 3
        last[axis] = -1
        on[axis][tuple(last)] = False
    return on[0], on[1], on[2], voxel_on


def components(aff, threshold=0.5, min_size=100):
    on_z, on_y, on_x, voxel_on = edge_masks(aff, threshold)
    shape = on_z.shape
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    strides = (shape[1] * shape[2], shape[2], 1)
    src = np.concatenate([idx[m] for m in (on_z, on_y, on_x)])
    dst = np.concatenate([idx[m] + s for m, s in zip((on_z, on_y, on_x), strides)])
    graph = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    size = np.bincount(comp)
    if voxel_on is None:    # affinity mode: a voxel without an on edge is background
        keep = size > max(int(min_size), 1)
    else:
        off = np.ones(size.size, bool)
        off[comp[voxel_on.ravel()]] = False
        keep = (size > max(int(min_size), 0)) & ~off
    # smallest linear index of every component = its first appearance in raster order
    first = np.empty(size.size, np.int64)
    first[comp[::-1]] = np.arange(n - 1, -1, -1, dtype=np.int64)   # the last write, the smallest index, stays
    kept = np.flatnonzero(keep)
    kept = kept[np.argsort(first[kept], kind="stable")]
    new_id = np.zeros(size.size, np.int32)
    new_id[kept] = np.arange(1, kept.size + 1, dtype=np.int32)
    return new_id[comp].reshape(shape), int(kept.size)


def affinities_of_foreground(on):
    """(3, D, H, W) float32 affinities of a boolean foreground: aff[c][v] = on[v] & on[v + e_c], 0 on the
    high faces. At any threshold in (0, 1] their components are the foreground's without its lone voxels."""
    on = np.asarray(on, dtype=bool)
    aff = np.zeros((3,) + on.shape, np.float32)
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        aff[axis][tuple(lo)] = on[tuple(lo)] & on[tuple(hi)]
    return aff


def drop_singletons(labels, k):
    """(labels, K) without the components of one voxel, the rest renumbered in the order they had: what
    affinity mode makes of a foreground labelling in raster order (scipy.ndimage.label's)."""
    sizes = np.bincount(labels.ravel(), minlength=k + 1)
    keep = sizes > 1
    keep[0] = False
    new_id = np.where(keep, np.cumsum(keep), 0).astype(np.int32)
    return new_id[labels], int(keep.sum())


def same_partition(a, b):
    """True iff two label arrays have the same background and a bijection between their ids."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    if not np.array_equal(a == 0, b == 0):
        return False
    pairs = np.unique(np.stack([a, b]), axis=1)
    return np.unique(pairs[0]).size == pairs.shape[1] == np.unique(pairs[1]).size
