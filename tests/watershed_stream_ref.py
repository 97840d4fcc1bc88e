"""
numpy model of the slab-by-slab watershed fragments (exaspim_watershed_stream_slab), step for step and
written from the definition. Only what the device carries crosses from one slab to the next: one plane of
provisional ids, one float32 plane of z affinities and two bits per (y, x).

  1. per slab [z0, z1): every voxel's steepest edge (watershed_ref's rules 1 and 2) among the edges inside the
     slab, the carried float32 plane as the -z edges of plane z0 (none for z0 = 0), and the slab's own channel-0
     values of plane z1 - 1 as +z edges (none for z1 = D, whatever they hold);
  2. the on edges inside the slab (rule 3); the z edges of plane z1 - 1 are no edges of the slab;
  3. the seam below the next slab, unless z1 = D: per (y, x) "eligible" (a > low) and "sure" (eligible and
     (a >= high or the edge is the steepest of its lower end));
  4. the seam above this slab, unless z0 = 0: the carried bits resolved with this slab's codes, on iff sure, or
     eligible and the first-plane voxel's steepest edge is -z;
  5. marks: above, a slab-local fragment with a resolved on edge to the carried plane (exact); below, one with an
     ELIGIBLE edge across the seam (conservative: whether it is switched on is the next slab's to say);
  6. a provisional id for every slab-local fragment that is marked or larger than max(min_size, 1) on its own,
     dense, in raster order of its first voxel, continuing the count; the union over ids of the two ends of every
     on seam edge, the smaller root winning;
  7. finish and apply as in components_stream_ref: sets with more than max(min_size, 1) voxels are numbered
     1 .. K in the order of their smallest id.

    fragments_streamed(aff, low, high, min_size, cuts, capacity=None)
        -> (labels int32 (D, H, W), K, provisional int32 (D, H, W), table int32, ids_used)

    slab_on_edges(aff, low, high, cuts) -> (on_z, on_y, on_x) boolean (D, H, W) of the whole volume, put together
        from the slabs' masks and the resolved seams: what watershed_ref.on_edges gives.
"""

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import watershed_ref

TO_LOW_Z, TO_HIGH_Z = 1, 6      # codes: 1 + the direction's place in watershed_ref.DIRECTIONS


def _find(parent, a):
    while parent[a] != a:
        a = parent[a]
    return a


def _slab_codes(slab, low, carry_aff, final):
    """int8 (d, H, W) steepest-edge codes of a float32 (3, d, H, W) slab."""
    inc = watershed_ref.incident(slab)           # NaN where an edge leaves the slab
    if carry_aff is not None:
        inc[0][0] = carry_aff                    # -z of plane 0: the carried plane
    if not final:
        inc[5][-1] = slab[0, -1]                 # +z of the last plane: its own channel-0 values
    with np.errstate(invalid="ignore"):
        eligible = inc > low
    value = np.where(eligible, inc, -np.inf)
    code = value.argmax(axis=0) + 1              # the first of equal values: -z, -y, -x, +x, +y, +z
    return np.where(eligible.any(axis=0), code, 0).astype(np.int8)


def _slab_masks(slab, low, high, code):
    """(on_z, on_y, on_x) boolean (d, H, W) inside the slab; the last plane's z edges are not the slab's."""
    on = []
    for axis in range(3):
        up = 1 + watershed_ref.DIRECTIONS.index((axis, +1))
        down = 1 + watershed_ref.DIRECTIONS.index((axis, -1))
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        e = np.zeros(slab.shape[1:], bool)
        with np.errstate(invalid="ignore"):
            eligible = slab[axis][lo] > low
            e[lo] = eligible & ((slab[axis][lo] >= high) | (code[lo] == up) | (code[hi] == down))
        on.append(e)
    return on


def _slabs(aff, low, high, cuts):
    """Yields (z0, z1, masks, seam_on, eligible, carried ids' seam): the per-slab steps 1 to 4."""
    aff = np.asarray(aff)
    if aff.dtype not in (np.dtype(np.float32), np.dtype(np.float16)) or aff.ndim != 4 or aff.shape[0] != 3:
        raise ValueError((aff.dtype, aff.shape))
    low, high = np.float32(low), np.float32(high)
    depth = aff.shape[1]
    bounds = [0] + [int(c) for c in cuts] + [depth]
    assert all(a < b for a, b in zip(bounds, bounds[1:])), bounds
    carry_aff = carry_elig = carry_sure = None
    for z0, z1 in zip(bounds, bounds[1:]):
        slab = aff[:, z0:z1].astype(np.float32)          # float16 widened exactly
        final = z1 == depth
        code = _slab_codes(slab, low, carry_aff, final)
        masks = _slab_masks(slab, low, high, code)
        seam_on = None
        if carry_elig is not None:
            seam_on = carry_sure | (carry_elig & (code[0] == TO_LOW_Z))
        elig = None
        if not final:
            with np.errstate(invalid="ignore"):
                elig = slab[0, -1] > low
                sure = elig & ((slab[0, -1] >= high) | (code[-1] == TO_HIGH_Z))
        yield z0, z1, masks, seam_on, elig
        if not final:
            carry_aff, carry_elig, carry_sure = slab[0, -1].copy(), elig, sure


def slab_on_edges(aff, low, high, cuts):
    shape = np.asarray(aff).shape[1:]
    on = [np.zeros(shape, bool) for _ in range(3)]
    for z0, z1, masks, seam_on, _ in _slabs(aff, low, high, cuts):
        for axis in range(3):
            on[axis][z0:z1] = masks[axis]
        if seam_on is not None:
            on[0][z0 - 1] = seam_on
    return tuple(on)


def fragments_streamed(aff, low=0.1, high=0.9999, min_size=0, cuts=(), capacity=None):
    depth, h, w = np.asarray(aff).shape[1:]
    min_eff = max(int(min_size), 1)
    parent = [0]     # union-find over provisional ids; id 0 is the background
    count = [0]
    provisional = np.zeros((depth, h, w), np.int32)
    carry_ids = None
    for z0, z1, (on_z, on_y, on_x), seam_on, elig in _slabs(aff, low, high, cuts):
        shape = on_z.shape
        n = int(np.prod(shape))
        idx = np.arange(n, dtype=np.int64).reshape(shape)
        strides = (shape[1] * shape[2], shape[2], 1)
        src = np.concatenate([idx[m] for m in (on_z, on_y, on_x)])
        dst = np.concatenate([idx[m] + s for m, s in zip((on_z, on_y, on_x), strides)])
        _, comp = connected_components(coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n)),
                                       directed=False)
        comp = comp.reshape(shape)
        size = np.bincount(comp.ravel())
        marked = np.zeros(size.size, bool)
        if seam_on is not None:
            marked[comp[0][seam_on]] = True       # above a seam: exact
        if elig is not None:
            marked[comp[-1][elig]] = True         # below a seam: every eligible edge, on or not
        wants = marked | (size > min_eff)
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
        if seam_on is not None:
            for a, b in zip(carry_ids[seam_on], labels[0][seam_on]):
                assert a > 0 and b > 0      # on implies eligible: the lower end was marked
                ra, rb = _find(parent, int(a)), _find(parent, int(b))
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
        carry_ids = labels[-1].copy()

    m = len(parent)
    root = np.array([_find(parent, i) for i in range(m)], np.int64)
    total = np.zeros(m, np.int64)
    np.add.at(total, root, np.array(count, np.int64))
    keep = (root == np.arange(m)) & (total > min_eff)
    keep[0] = False
    final = np.zeros(m, np.int32)
    final[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    table = final[root]
    return table[provisional], int(keep.sum()), provisional, table, m - 1
