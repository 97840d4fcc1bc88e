"""
Host oracles for label_pieces (no GPU), written from the definition in include/exaspim_affinity.h:
a voxel is foreground iff its label is in 1..K; a piece is a maximal 26-connected set of foreground voxels with one
label; a piece of at least dust_threshold voxels is kept, the others are dust; kept pieces are numbered 1..P in
ascending order of their first voxel (the smallest linear index).

(A) flood_fill: a plain flood fill over the 26 neighbours, voxel by voxel in linear order.
(B) by_label: scipy.ndimage.label per label with a 3 x 3 x 3 structure, renumbered by first voxel.

Both return (pieces int32 volume, piece_label int32 (P,), piece_size int64 (P,), piece_first int32 (P,), dust count);
tests/test_pieces_ref_cpu.py holds them to each other.
"""

import numpy as np
from scipy import ndimage

FULL = np.ones((3, 3, 3), dtype=bool)
OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
# the 13 of them that come before a voxel in linear order
EARLIER = [o for o in OFFSETS if o < (0, 0, 0)]


def foreground(labels, k):
    labels = np.asarray(labels)
    return np.where((labels >= 1) & (labels <= k), labels, 0).astype(np.int64)


def _numbered(shape, found, dust_threshold):
    """found: (first voxel, label, flat indices) per piece, any order."""
    pieces = np.zeros(int(np.prod(shape)), dtype=np.int32)
    kept = sorted((f for f in found if len(f[2]) >= dust_threshold), key=lambda f: f[0])
    for number, (_, _, voxels) in enumerate(kept, start=1):
        pieces[voxels] = number
    return (pieces.reshape(shape), np.array([f[1] for f in kept], dtype=np.int32),
            np.array([len(f[2]) for f in kept], dtype=np.int64), np.array([f[0] for f in kept], dtype=np.int32),
            len(found) - len(kept))


def flood_fill(labels, k, dust_threshold=0):
    """Oracle (A)."""
    fg = foreground(labels, k)
    d, h, w = fg.shape
    seen = np.zeros(fg.shape, dtype=bool)
    found = []
    for z, y, x in zip(*np.nonzero(fg)):      # C order: the first voxel of a piece is met first
        if seen[z, y, x]:
            continue
        value = fg[z, y, x]
        seen[z, y, x] = True
        stack, voxels = [(z, y, x)], []
        while stack:
            cz, cy, cx = stack.pop()
            voxels.append((cz * h + cy) * w + cx)
            for dz, dy, dx in OFFSETS:
                nz, ny, nx = cz + dz, cy + dy, cx + dx
                if 0 <= nz < d and 0 <= ny < h and 0 <= nx < w and not seen[nz, ny, nx] and fg[nz, ny, nx] == value:
                    seen[nz, ny, nx] = True
                    stack.append((nz, ny, nx))
        found.append((int((z * h + y) * w + x), int(value), np.array(sorted(voxels), dtype=np.int64)))
    return _numbered(fg.shape, found, dust_threshold)


def by_label(labels, k, dust_threshold=0):
    """Oracle (B)."""
    fg = foreground(labels, k)
    found = []
    for value in np.unique(fg[fg > 0]):
        components, count = ndimage.label(fg == value, structure=FULL)
        inside = np.flatnonzero(components)      # ascending linear indices: the sort below only has to be stable
        number = components.reshape(-1)[inside]
        order = np.argsort(number, kind="stable")
        bounds = np.searchsorted(number[order], np.arange(1, count + 2))
        for c in range(count):
            voxels = inside[order[bounds[c]:bounds[c + 1]]]
            found.append((int(voxels[0]), int(value), voxels))
    return _numbered(fg.shape, found, dust_threshold)


def random_volume(seed, shape, k=3, fill=0.35):
    """Seeded labels in -1..k+1: even seeds voxel noise, odd seeds blocks of 2 voxels so that pieces go deep."""
    rng = np.random.default_rng(seed)
    if seed % 2:
        coarse = tuple(-(-s // 2) for s in shape)
        values = np.where(rng.random(coarse) < fill, rng.integers(-1, k + 2, size=coarse), 0)
        values = np.kron(values, np.ones((2, 2, 2), dtype=np.int64))[:shape[0], :shape[1], :shape[2]]
    else:
        values = np.where(rng.random(shape) < fill, rng.integers(-1, k + 2, size=shape), 0)
    return np.ascontiguousarray(values, dtype=np.int32)


def seam_pair(offset, second_label=1, shape=(16, 16, 64)):
    """Two voxels, one step along the offset apart, that straddle the tile corner z = 7|8, y = 7|8, x = 31|32 on
    every axis the offset moves along; on the other axes both lie on the corner's low side."""
    labels = np.zeros(shape, dtype=np.int32)
    a = tuple(c if o < 0 else c - 1 for c, o in zip((8, 8, 32), offset))      # o < 0: from the high side down
    b = tuple(p + o for p, o in zip(a, offset))
    labels[a] = 1
    labels[b] = second_label
    return labels


def crafted():
    """name -> (labels, K, dust_threshold, the number of kept pieces or None)."""
    cases = {}
    for offset in EARLIER:
        cases[f"seam pair {offset}"] = (seam_pair(offset), 1, 0, 1)
        cases[f"seam pair {offset}, two labels"] = (seam_pair(offset, 2), 2, 0, 2)
    shape = (5, 6, 7)
    parity = np.indices(shape).sum(axis=0) % 2
    cases["a two-label checkerboard"] = ((parity + 1).astype(np.int32), 2, 0, 2)
    even = np.zeros(shape, dtype=np.int32)
    even[::2, ::2, ::2] = 1
    cases["all-even voxels"] = (even, 1, 0, 3 * 3 * 4)
    gap = np.zeros((4, 9, 5), dtype=np.int32)
    gap[:, :4] = 1
    gap[:, 5:] = 1
    cases["one plane of background between"] = (gap, 1, 0, 2)
    wall = gap.copy()
    wall[:, 4] = 2
    cases["one plane of another label between"] = (wall, 2, 0, 3)
    cases["a diagonal snake"] = (snake((20, 20, 70)), 1, 0, 1)
    mixed = np.zeros((3, 4, 6), dtype=np.int32)
    mixed[0, 0, :2] = 5
    mixed[1, 1, 2:4] = -2
    mixed[2, 2, :3] = 2
    mixed[0, 3, 4:] = 1
    cases["labels above K and negative"] = (mixed, 2, 0, 2)
    cases["K = 0"] = (mixed, 0, 0, 0)
    cases["an empty volume"] = (np.zeros((3, 4, 5), dtype=np.int32), 3, 0, 0)
    cases["one voxel"] = (np.ones((1, 1, 1), dtype=np.int32), 1, 0, 1)
    for t, kept in ((0, 3), (1, 3), (4, 2), (5, 1), (6, 0)):
        cases[f"dust at {t}"] = (dust_volume(4), 1, t, kept)      # sizes 3, 4, 5
    return cases


def snake(shape):
    """A one-voxel-wide path of label 1 that steps diagonally through the volume and turns at the faces."""
    labels = np.zeros(shape, dtype=np.int32)
    z = y = x = 0
    sz = sy = 1
    for x in range(shape[2]):
        labels[z, y, x] = 1
        if not 0 <= z + sz < shape[0]:
            sz = -sz
        if x % 3 == 0:
            if not 0 <= y + sy < shape[1]:
                sy = -sy
            y += sy
        z += sz
    return labels


def dust_volume(t):
    """Three bars of label 1 of t - 1, t and t + 1 voxels, apart from each other, the largest first."""
    labels = np.zeros((3, 5, max(40, t + 21)), dtype=np.int32)
    labels[0, 0, :t + 1] = 1
    labels[2, 2, 10:10 + t - 1] = 1
    labels[1, 4, 20:20 + t] = 1
    return labels
