"""
numpy model of the slab-by-slab components (exaspim_components_stream_*), step for step:

  1. per slab [z0, z1): the slab-local components (z edges of the slab's last plane dropped inside
     the slab, remembered as the seam's bits unless the plane is the volume's last); a provisional id
     for every local component that is larger than min_size on its own or has an on edge across a
     seam -- dense, in raster order of the local component's first voxel, continuing the previous
     slab's count -- with its voxel count in a table;
  2. per seam: union, over ids, of the two ends of every on z edge from plane z0 - 1 to plane z0,
     the smaller root winning;
  3. finish: counts summed per root, roots with count > min_size (floors: 1 in affinity mode, 0 in
     foreground mode) numbered 1 .. K in id order: table[id] -> final label, table[0] = 0;
  4. apply: labels = table[provisional].

    components_streamed(aff, threshold, min_size, cuts, capacity=None)
        -> (labels int32 (D, H, W), K, provisional int32 (D, H, W), table int32)

aff as in components_ref.components; cuts are the interior z positions where one slab ends and the
next one starts. capacity: raises OverflowError when more ids are needed. Only what crosses from one
slab to the next is carried: one plane of ids and one plane of bits.
"""

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import components_ref


def _find(parent, a):
    while parent[a] != a:
        a = parent[a]
    return a


def components_streamed(aff, threshold=0.5, min_size=100, cuts=(), capacity=None):
    aff = np.asarray(aff)
    foreground = aff.ndim == 3
    depth = aff.shape[-3]
    h, w = aff.shape[-2:]
    floor = 0 if foreground else 1
    min_eff = max(int(min_size), floor)
    bounds = [0] + [int(c) for c in cuts] + [depth]
    assert all(a < b for a, b in zip(bounds, bounds[1:])), bounds

    parent = [0]     # union-find over provisional ids; id 0 is the background
    count = [0]
    provisional = np.zeros((depth, h, w), np.int32)
    carry_ids = carry_bits = None
    for z0, z1 in zip(bounds, bounds[1:]):
        slab = aff[..., z0:z1, :, :]
        on_z, on_y, on_x, voxel_on = components_ref.edge_masks(slab, threshold)   # last plane's z edges off
        shape = on_z.shape
        n = int(np.prod(shape))
        # the seam below this slab: its bits, taken from the data the slab itself holds
        seam_bits = None
        if z1 < depth:
            if foreground:
                seam_bits = voxel_on[-1].copy()
            else:
                with np.errstate(invalid="ignore"):
                    seam_bits = slab[0, -1].astype(np.float32) >= np.float32(threshold)
        idx = np.arange(n, dtype=np.int64).reshape(shape)
        strides = (shape[1] * shape[2], shape[2], 1)
        src = np.concatenate([idx[m] for m in (on_z, on_y, on_x)])
        dst = np.concatenate([idx[m] + s for m, s in zip((on_z, on_y, on_x), strides)])
        _, comp = connected_components(coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n)),
                                       directed=False)
        comp = comp.reshape(shape)
        size = np.bincount(comp.ravel())
        on = np.ones(shape, bool) if voxel_on is None else voxel_on
        # which local components have an on edge across a seam
        marked = np.zeros(size.size, bool)
        seam_edge = None
        if carry_bits is not None:
            seam_edge = carry_bits & on[0]
            marked[comp[0][seam_edge]] = True
        if seam_bits is not None:
            marked[comp[-1][seam_bits]] = True
        is_on = np.zeros(size.size, bool)
        is_on[comp[on]] = True
        wants = is_on & (marked | (size > min_eff))
        # ids in raster order of the first voxel
        first = np.empty(size.size, np.int64)
        first[comp.ravel()[::-1]] = np.arange(n - 1, -1, -1, dtype=np.int64)
        chosen = np.flatnonzero(wants)
        chosen = chosen[np.argsort(first[chosen], kind="stable")]
        base = len(parent) - 1
        if capacity is not None and base + chosen.size > capacity:
            raise OverflowError(f"{base + chosen.size} provisional ids, capacity {capacity}")
        ids = np.zeros(size.size, np.int32)
        ids[chosen] = base + 1 + np.arange(chosen.size, dtype=np.int32)
        parent.extend(range(base + 1, base + 1 + chosen.size))
        count.extend(int(size[c]) for c in chosen)
        labels = ids[comp]
        provisional[z0:z1] = labels
        # the seam above this slab
        if seam_edge is not None:
            for a, b in zip(carry_ids[seam_edge], labels[0][seam_edge]):
                assert a > 0 and b > 0
                ra, rb = _find(parent, int(a)), _find(parent, int(b))
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
        carry_ids, carry_bits = labels[-1].copy(), seam_bits

    # finish
    m = len(parent)
    root = np.array([_find(parent, i) for i in range(m)], np.int64)
    total = np.zeros(m, np.int64)
    np.add.at(total, root, np.array(count, np.int64))
    keep = (root == np.arange(m)) & (total > min_eff)
    keep[0] = False
    final = np.zeros(m, np.int32)
    final[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    table = final[root]
    return table[provisional], int(keep.sum()), provisional, table
