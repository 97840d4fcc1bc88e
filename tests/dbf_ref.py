"""
CPU oracle of the distance-to-boundary field and the segment table, numpy and scipy only,
written from the definition in include/exaspim_affinity.h and not from the kernels:

  brute_force   every voxel against every voxel of another label (and the border layer), O(n^2);
  per_label     scipy.ndimage.distance_transform_edt(return_indices=True) per label on its bounding box
                plus a margin; the squared distance comes from the integer index differences it returns,
                never from its float distances;
  segment_table numpy: bincount, ndimage.find_objects and a stable argmax (and segment_table_sorted, the
                same from one stable sort, for volumes with many thousands of labels);
  tiled_rows    a tall volume of small blocks between zero rows and its dbf, composed from per_label of the
                blocks: for volumes of 10^7 voxels, where a whole-volume EDT is too slow.

tests/test_dbf_ref_cpu.py holds the first two to each other exactly, and tiled_rows to per_label.
"""

import numpy as np
from scipy import ndimage

DBF_INF = 2**31 - 1


def brute_force(labels, black_border=False):
    """dbf by the definition: the minimum over all voxels of another label, and over the border layer."""
    labels = np.asarray(labels)
    shape = labels.shape
    coords = np.indices(shape).reshape(3, -1).T.astype(np.int64)
    flat = labels.reshape(-1)
    out = np.zeros(flat.size, dtype=np.int64)
    for i in np.flatnonzero(flat > 0):
        best = DBF_INF
        other = flat != flat[i]
        if other.any():
            best = int(((coords[other] - coords[i]) ** 2).sum(axis=1).min())
        if black_border:
            for axis in range(3):
                c, n = int(coords[i, axis]), shape[axis]
                best = min(best, (c + 1) ** 2, (n - c) ** 2)
        out[i] = best
    return out.reshape(shape).astype(np.int32)


def per_label(labels, black_border=False, margin=1, on_label=None):
    """dbf from a per-label scipy EDT with indices; exact, since only the integer indices are used.
    on_label(done, total), if given, is called after every label (tools/dbf_rate.py's progress and budget)."""
    labels = np.asarray(labels)
    if black_border:
        padded = np.zeros(tuple(s + 2 for s in labels.shape), dtype=labels.dtype)
        padded[1:-1, 1:-1, 1:-1] = labels
        return np.ascontiguousarray(per_label(padded, False, margin, on_label)[1:-1, 1:-1, 1:-1])
    out = np.zeros(labels.shape, dtype=np.int32)
    values = np.unique(labels)
    values = values[values > 0]
    if values.size == 0:
        return out
    # find_objects wants small positive ids: rank the values (labels may be as large as 2^31 - 1)
    ranks = np.searchsorted(values, labels).astype(np.int64) + 1
    ranks[labels <= 0] = 0
    for rank, box in enumerate(ndimage.find_objects(ranks), start=1):
        grown = tuple(slice(max(s.start - margin, 0), min(s.stop + margin, n)) for s, n in zip(box, labels.shape))
        inside = ranks[grown] == rank
        if inside.all():      # the label fills its grown box: the box is the volume, nothing bounds it
            assert inside.shape == labels.shape
            out[grown][inside] = DBF_INF
            continue
        idx = ndimage.distance_transform_edt(inside, return_distances=False, return_indices=True)
        d2 = np.zeros(inside.shape, dtype=np.int64)
        for axis in range(3):      # the nearest outside voxel's index minus the voxel's own, per axis
            along = [1, 1, 1]
            along[axis] = -1
            d = idx[axis].astype(np.int64) - np.arange(inside.shape[axis]).reshape(along)
            d2 += d * d
        view = out[grown]
        view[inside] = d2[inside].astype(np.int32)
        if on_label is not None:
            on_label(rank, len(values))
    return out


def segment_table(labels, dbf=None, n_labels=None):
    """(sizes, boxes, peak, peak_index) with n_labels + 1 rows each, by the definition."""
    labels = np.asarray(labels)
    k = max(int(labels.max(initial=0)), 0) if n_labels is None else int(n_labels)
    flat = labels.reshape(-1).astype(np.int64)
    known = (flat >= 0) & (flat <= k)
    sizes = np.bincount(flat[known], minlength=k + 1).astype(np.int64)
    boxes = np.zeros((k + 1, 6), dtype=np.int32)
    peak = np.zeros(k + 1, dtype=np.int32)
    peak_index = np.full(k + 1, -1, dtype=np.int32)
    field = np.zeros(flat.size, dtype=np.int64) if dbf is None else np.asarray(dbf).reshape(-1).astype(np.int64)
    clean = np.where((labels > 0) & (labels <= k), labels, 0)
    for lab, box in enumerate(ndimage.find_objects(clean, max_label=k), start=1):
        if box is None:
            continue
        boxes[lab] = [s.start for s in box] + [s.stop for s in box]
        where = np.flatnonzero(flat == lab)              # ascending linear indices
        best = int(np.argmax(field[where]))               # the first of equal maxima
        peak[lab] = field[where][best]
        peak_index[lab] = where[best]
    return sizes, boxes, peak, peak_index


def segment_table_sorted(labels, dbf=None, n_labels=None):
    """The same table from one stable sort by label and reduceat: for volumes with many thousands of labels,
    where segment_table's loop over the labels is too slow. Held to segment_table in tests/test_dbf_ref_cpu.py."""
    labels = np.asarray(labels)
    k = max(int(labels.max(initial=0)), 0) if n_labels is None else int(n_labels)
    flat = labels.reshape(-1).astype(np.int64)
    sizes = np.bincount(flat[(flat >= 0) & (flat <= k)], minlength=k + 1).astype(np.int64)
    boxes = np.zeros((k + 1, 6), dtype=np.int32)
    peak = np.zeros(k + 1, dtype=np.int32)
    peak_index = np.full(k + 1, -1, dtype=np.int32)
    keep = np.flatnonzero((flat > 0) & (flat <= k))              # ascending linear indices
    if keep.size == 0:
        return sizes, boxes, peak, peak_index
    order = keep[np.argsort(flat[keep], kind="stable")]          # by label, then by linear index
    sorted_labels = flat[order]
    starts = np.flatnonzero(np.r_[True, sorted_labels[1:] != sorted_labels[:-1]])
    present = sorted_labels[starts]
    coords = np.unravel_index(order, labels.shape)
    for axis in range(3):
        boxes[present, axis] = np.minimum.reduceat(coords[axis], starts)
        boxes[present, 3 + axis] = np.maximum.reduceat(coords[axis], starts) + 1
    field = np.zeros(order.size, dtype=np.int64) if dbf is None else np.asarray(dbf).reshape(-1)[order].astype(np.int64)
    best = np.maximum.reduceat(field, starts)
    peak[present] = best
    at_peak = field == np.repeat(best, np.diff(np.r_[starts, order.size]))
    peak_index[present] = np.minimum.reduceat(np.where(at_peak, order, flat.size), starts)
    return sizes, boxes, peak, peak_index


def tiled_rows(blocks, choice, black_border=False):
    """
    (labels, expected): a tall volume composed of small blocks, and its dbf composed of theirs; for volumes
    too large for per_label. blocks are (D, bh, W) label arrays of one shape. The volume is one zero row
    (a y index, over all z and x), then for every c in choice blocks[c] followed by one zero row:
    H = 1 + (bh + 1) * len(choice). A block's field is per_label of the block between two zero rows.
    Exact in both border modes: whatever lies beyond a zero row is farther away than that row's voxel at the
    same (z, x), which is of another label, and a block's z and x faces are the volume's own.
    tests/test_dbf_ref_cpu.py holds it to per_label of the whole volume.
    """
    blocks = np.stack([np.asarray(b, dtype=np.int32) for b in blocks])
    between = ((0, 0), (1, 1), (0, 0))
    fields = np.stack([per_label(np.pad(b, between), black_border)[:, 1:-1, :] for b in blocks])
    choice = np.asarray(choice, dtype=np.int64)
    _, d, bh, w = blocks.shape

    def compose(parts):
        rows = np.pad(parts, ((0, 0), (0, 0), (0, 1), (0, 0)))[choice]          # every block with its zero row
        tall = np.moveaxis(rows, 0, 1).reshape(d, choice.size * (bh + 1), w)
        return np.ascontiguousarray(np.pad(tall, ((0, 0), (1, 0), (0, 0))))

    return compose(blocks), compose(fields)


def stretched_labels(rng, shape, top=3, longest=40):
    """Random labels in 0 .. top along x in runs of random length 1 .. longest: runs cross every chunk."""
    n = int(np.prod(shape))
    lengths = rng.integers(1, longest + 1, size=n)
    values = rng.integers(0, top + 1, size=n)
    return np.repeat(values, lengths)[:n].reshape(shape).astype(np.int32)
