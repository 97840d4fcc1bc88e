"""
Transforms under which the label kernels' definitions do not change, in
plain numpy, and the seeded inputs the CPU and the GPU symmetry tests share. No GPU here.

The 48 symmetries of the box. A symmetry is (perm, flips): new axis a is old axis perm[a], read backwards
iff flips[a].
    apply_volume(sym, v)              transpose, then flip, C-contiguous
    apply_affinities(sym, aff, fill)  channel a is old channel perm[a]; under a flip of axis a channel a is
                                      flipped and shifted by one (the edge between new i and i + 1 is the old
                                      edge stored at n - 2 - i) and its new last entry, which the convention
                                      ignores, is "fill", a value that would be on if it were read
    apply_indices(sym, idx, shape)    C-order linear indices of the old shape -> of the new one, -1 stays
    apply_boxes(sym, boxes, shape)    half-open (z0, y0, x0, z1, y1, x1) rows; all-zero rows stay
    inverse(sym)                      the symmetry that undoes sym
Translation. embed_volume / embed_affinities put a volume at "offset" in a background volume with "tail" more
voxels on the high side; crop takes it back; shift_indices and shift_boxes move what points into it. The
entries of channel c at the block's last index along axis c become real edges into the padding: they are set
to the padding's value.
Relabelling. relabel_volume, relabel_rows and relabel_edges rename 1 .. K through a table; label_maps gives
the three maps the tests use.
Comparison. same_labelling (same partition and same K), correspondence (the label found at the same voxel)
and graph_dict ({(u, v): (count, sum)}, optionally renamed through a correspondence).
"""

import itertools

import numpy as np

import components_ref
import holes_ref
import pieces_ref

TILE = (8, 8, 32)
LDS_SLOTS = 2048      # slots of the region graph's table in LDS: ids equal modulo this share a home slot

SYMMETRIES = [(perm, flips) for perm in itertools.permutations(range(3))
              for flips in itertools.product((False, True), repeat=3)]
IDENTITY = ((0, 1, 2), (False, False, False))
# the six axis permutations and the eight flips: 13 symmetries besides the identity, which generate the group
GENERATORS = [s for s in SYMMETRIES if s[1] == IDENTITY[1] or s[0] == IDENTITY[0]]


def name(sym):
    perm, flips = sym
    return "".join("zyx"[p] for p in perm) + "".join("-" if f else "+" for f in flips)


def inverse(sym):
    perm, flips = sym
    back = tuple(int(a) for a in np.argsort(perm))
    return back, tuple(flips[a] for a in back)


def new_shape(sym, shape):
    return tuple(shape[p] for p in sym[0])


# ---- the box symmetries ----------------------------------------------------------------------------------
def apply_volume(sym, v):
    perm, flips = sym
    v = np.asarray(v)
    assert v.ndim == 3
    out = np.transpose(v, perm)
    axes = tuple(a for a in range(3) if flips[a])
    if axes:
        out = np.flip(out, axes)
    return np.ascontiguousarray(out)


def set_ignored(aff, fill):
    """aff with the entries the convention ignores (channel c at the last index along axis c) set to fill."""
    out = np.array(aff, order="C")
    for c in range(3):
        last = [slice(None)] * 3
        last[c] = -1
        out[c][tuple(last)] = fill
    return out


def apply_affinities(sym, aff, fill=1.0):
    perm, flips = sym
    aff = np.asarray(aff)
    assert aff.ndim == 4 and aff.shape[0] == 3
    out = np.empty((3,) + new_shape(sym, aff.shape[1:]), dtype=aff.dtype)
    for a in range(3):
        ch = apply_volume(sym, aff[perm[a]])
        if flips[a]:
            # after the plain flip index i holds the old entry n - 1 - i; the edge i -- i + 1 is the old entry n - 2 - i
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            last = [slice(None)] * 3
            lo[a], hi[a], last[a] = slice(0, -1), slice(1, None), -1
            moved = np.empty_like(ch)
            moved[tuple(lo)] = ch[tuple(hi)]
            moved[tuple(last)] = fill
            ch = moved
        out[a] = ch
    return out


def apply_indices(sym, idx, shape):
    perm, flips = sym
    idx = np.asarray(idx)
    out = np.full(idx.shape, -1, dtype=idx.dtype)
    ok = idx >= 0
    old = np.unravel_index(idx[ok].astype(np.int64), shape)
    new = [shape[perm[a]] - 1 - old[perm[a]] if flips[a] else old[perm[a]] for a in range(3)]
    out[ok] = np.ravel_multi_index(new, new_shape(sym, shape)).astype(idx.dtype)
    return out


def apply_boxes(sym, boxes, shape):
    perm, flips = sym
    boxes = np.asarray(boxes)
    out = np.zeros_like(boxes)
    present = boxes[:, 3:].min(axis=1) > 0      # an absent label's row is all zeros, and stays so
    for a in range(3):
        lo, hi, n = boxes[:, perm[a]], boxes[:, 3 + perm[a]], shape[perm[a]]
        out[:, a] = np.where(present, n - hi if flips[a] else lo, 0)
        out[:, 3 + a] = np.where(present, n - lo if flips[a] else hi, 0)
    return out


# ---- translation -----------------------------------------------------------------------------------------
def padded_shape(shape, offset, tail):
    return tuple(o + s + t for o, s, t in zip(offset, shape, tail))


def _block(offset, shape):
    return tuple(slice(o, o + s) for o, s in zip(offset, shape))


def embed_volume(v, offset, tail, fill=0):
    v = np.asarray(v)
    out = np.full(padded_shape(v.shape, offset, tail), fill, dtype=v.dtype)
    out[_block(offset, v.shape)] = v
    return out


def embed_affinities(aff, offset, tail, off=0.0):
    aff = np.asarray(aff)
    out = np.full((3,) + padded_shape(aff.shape[1:], offset, tail), off, dtype=aff.dtype)
    out[(slice(None),) + _block(offset, aff.shape[1:])] = set_ignored(aff, off)
    return out


def crop(v, offset, shape):
    v = np.asarray(v)
    return np.ascontiguousarray(v[(Ellipsis,) + _block(offset, shape)])


def shift_indices(idx, shape, offset, tail):
    idx = np.asarray(idx)
    out = np.full(idx.shape, -1, dtype=idx.dtype)
    ok = idx >= 0
    old = np.unravel_index(idx[ok].astype(np.int64), shape)
    out[ok] = np.ravel_multi_index([c + o for c, o in zip(old, offset)],
                                   padded_shape(shape, offset, tail)).astype(idx.dtype)
    return out


def shift_boxes(boxes, offset):
    boxes = np.asarray(boxes)
    present = boxes[:, 3:].min(axis=1) > 0
    return np.where(present[:, None], boxes + np.asarray(tuple(offset) * 2, dtype=boxes.dtype), 0)


# ---- relabelling -----------------------------------------------------------------------------------------
def label_maps(k, seed=0):
    """{name: table int32 (k + 1,)}, table[0] = 0 and table[1:] injective into 1 .. K'."""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, k + 1)
    maps = {
        "permutation": rng.permutation(ids),
        "sparse": np.sort(rng.choice(np.arange(1, 5 * LDS_SLOTS + 1), size=k, replace=False))[rng.permutation(k)],
        "one_home_slot": LDS_SLOTS * (ids - 1) + 1,
    }
    return {key: np.concatenate([[0], value]).astype(np.int32) for key, value in maps.items()}


def relabel_volume(labels, table):
    labels = np.asarray(labels)
    assert labels.min() >= 0 and labels.max() < len(table)
    return np.ascontiguousarray(np.asarray(table)[labels], dtype=labels.dtype)


def relabel_rows(rows, table, absent):
    """A per-label output or input with k + 1 rows -> K' + 1 rows: row table[L] is row L, the others "absent"."""
    rows = np.asarray(rows)
    table = np.asarray(table)
    assert len(rows) == len(table)
    out = np.empty((int(table.max()) + 1,) + rows.shape[1:], dtype=rows.dtype)
    out[...] = absent
    out[table] = rows      # table[0] = 0: row 0 stays row 0
    return out


def relabel_edges(edges, table, *columns):
    """(edges renamed with lo < hi restored and sorted by (lo, hi), the columns in the same order)."""
    renamed = np.sort(np.asarray(table)[np.asarray(edges)], axis=1).astype(np.int32).reshape(-1, 2)
    order = np.lexsort((renamed[:, 1], renamed[:, 0]))
    return (np.ascontiguousarray(renamed[order]),) + tuple(np.asarray(c)[order] for c in columns)


# ---- comparison ------------------------------------------------------------------------------------------
def same_labelling(a, b):
    """The same partition (background included) under the same number of ids 1 .. K."""
    return components_ref.same_partition(a, b) and int(np.max(a, initial=0)) == int(np.max(b, initial=0))


def correspondence(a, b):
    """table with table[id in a] = the id b holds at the same voxels; a and b must be the same partition."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    assert components_ref.same_partition(a, b)
    table = np.zeros(int(a.max(initial=0)) + 1, dtype=np.int64)
    table[a] = b
    return table


def graph_dict(edges, counts, sums, table=None):
    """{(u, v): (count, sum)} with u < v, the ids renamed through table (a correspondence) if given."""
    edges = np.asarray(edges).reshape(-1, 2)
    if table is not None:
        edges = np.asarray(table)[edges]
    out = {}
    for (u, v), c, s in zip(edges.tolist(), np.asarray(counts).tolist(), np.asarray(sums).tolist()):
        key = (min(u, v), max(u, v))
        assert key not in out and u != v
        out[key] = (int(c), int(s))
    return out


# ---- the seeded inputs, and what the tests assert about them --------------------------------------------
DUST = 40      # the dust threshold the tests use besides 0


def label_volume(shape, seed, top=12, block=4, density=0.08):
    """int32 labels 0 .. K: a field that is constant on block^3 cells, a fraction "density" of it knocked out
    to background, the ids that are left renumbered 1 .. K. Read-only."""
    rng = np.random.default_rng(seed)
    labels = holes_ref.blocky(rng, shape, top, block)
    labels[rng.random(shape) < density] = 0
    values = np.unique(labels[labels > 0])
    out = np.where(labels > 0, np.searchsorted(values, labels) + 1, 0).astype(np.int32)
    out.setflags(write=False)
    return out


def label_facts(labels, sources, dust=DUST):
    """What a label volume offers the relations, as a dict of numbers; the tests assert on them."""
    labels = np.asarray(labels)
    k = int(labels.max())
    z, y, x = np.nonzero(labels)
    ids = labels[z, y, x]
    spans = []      # per axis: the most tiles one label is present in along it
    for coord, t in zip((z, y, x), TILE):
        pairs = np.unique(np.stack([ids, coord // t]), axis=1)
        spans.append(int(np.bincount(pairs[0]).max()))
    touching = 0
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        a, b = labels[tuple(lo)], labels[tuple(hi)]
        touching += int(((a > 0) & (b > 0) & (a != b)).sum())
    filled, stats = holes_ref.by_components(labels)
    pieces, piece_label, piece_size, _, _ = pieces_ref.by_label(labels, k, 0)
    per_label = np.bincount(piece_label, minlength=k + 1)
    split_with_dust = sorted({int(l) for l, s in zip(piece_label, piece_size) if per_label[l] >= 2 and s < dust})
    source_piece = np.zeros(k + 1, dtype=np.int64)
    has = np.asarray(sources) >= 0
    source_piece[has] = pieces.reshape(-1)[np.asarray(sources)[has]]
    unreachable = int(((labels > 0) & (pieces != source_piece[labels])).sum())
    return dict(k=k, tiles_spanned=min(spans), touching_faces=touching, holes=stats["filled"],
                hole_voxels=int((filled != labels).sum()), split_labels_with_dust=len(split_with_dust),
                dust_pieces=int((piece_size < dust).sum()), kept_pieces=int((piece_size >= dust).sum()),
                unreachable=unreachable)


def watershed_affinities(shape, seed, fill=1.0):
    """float32 (3,) + shape: a seeded permutation of the distinct values k / N, k = 0 .. N - 1, so that no two
    edges tie; the ignored entries hold "fill". Read-only."""
    n = 3 * int(np.prod(shape))
    assert n < 1 << 24      # k / N are distinct float32 values
    values = (np.random.default_rng(seed).permutation(n) / np.float64(n)).astype(np.float32)
    assert np.unique(values).size == n
    out = set_ignored(values.reshape((3,) + tuple(shape)), fill)
    out.setflags(write=False)
    return out


def component_affinities(shape, seed, on_fraction=0.27, fill=1.0):
    """(aff float32 (3,) + shape, threshold): smoothed noise and the threshold that switches on_fraction of
    its entries on, a little above bond percolation (0.249 on the cubic lattice). Read-only."""
    from scipy import ndimage

    u = np.random.default_rng(seed).random((3,) + tuple(shape)).astype(np.float32)
    u = ndimage.uniform_filter(u, size=(1, 2, 2, 2), mode="nearest").astype(np.float32)
    threshold = float(np.float32(np.quantile(u, 1.0 - on_fraction)))
    out = set_ignored(u, fill)
    out.setflags(write=False)
    return out, threshold


def tiles_of_largest(labels):
    """The number of distinct tiles the largest component occupies."""
    sizes = np.bincount(np.asarray(labels).ravel())
    sizes[0] = 0
    z, y, x = np.nonzero(labels == sizes.argmax())
    return np.unique(np.stack([z // TILE[0], y // TILE[1], x // TILE[2]]), axis=1).shape[1]


# ---- a transform as an object: the relations below are written once for symmetries and translations ------
class BoxSymmetry:
    """One of SYMMETRIES acting on volumes of "shape". C order is not kept: what a tie rule picks may move."""

    keeps_order = False

    def __init__(self, sym, shape):
        self.sym, self.shape, self.inv = sym, tuple(shape), inverse(sym)
        self.name = name(sym)
        self.padding = 0

    def volume(self, v, fill=0):
        return apply_volume(self.sym, v)

    def affinities(self, aff, on=1.0, off=0.0):
        return apply_affinities(self.sym, aff, on)

    def indices(self, idx):
        return apply_indices(self.sym, idx, self.shape)

    def boxes(self, boxes):
        return apply_boxes(self.sym, boxes, self.shape)

    def back(self, v):
        return apply_volume(self.inv, v)

    def back_indices(self, idx):
        return apply_indices(self.inv, idx, new_shape(self.sym, self.shape))


class Translation:
    """The volume at "offset" inside a background volume with "tail" more voxels on the high side. C order
    is kept, so what a smallest-index rule picks moves with the volume."""

    keeps_order = True

    def __init__(self, offset, tail, shape):
        self.offset, self.tail, self.shape = tuple(offset), tuple(tail), tuple(shape)
        self.name = f"+{self.offset} tail {self.tail}"
        self.padding = int(np.prod(padded_shape(shape, offset, tail))) - int(np.prod(shape))

    def volume(self, v, fill=0):
        return embed_volume(v, self.offset, self.tail, fill)

    def affinities(self, aff, on=1.0, off=0.0):
        return embed_affinities(aff, self.offset, self.tail, off)

    def indices(self, idx):
        return shift_indices(idx, self.shape, self.offset, self.tail)

    def boxes(self, boxes):
        return shift_boxes(boxes, self.offset)

    def back(self, v):
        return crop(v, self.offset, self.shape)

    def back_indices(self, idx):
        idx = np.asarray(idx)
        out = np.full(idx.shape, -1, dtype=idx.dtype)
        ok = idx >= 0
        there = np.unravel_index(idx[ok].astype(np.int64), padded_shape(self.shape, self.offset, self.tail))
        here = [c - o for c, o in zip(there, self.offset)]
        assert all(((c >= 0) & (c < n)).all() for c, n in zip(here, self.shape)), "an index points into the padding"
        out[ok] = np.ravel_multi_index(here, self.shape).astype(idx.dtype)
        return out


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def _same_outside(out, back, value=0):
    """Whatever a transform added around the volume holds "value": as many other entries in the whole
    output as in the part taken back."""
    assert int((np.asarray(out) != value).sum()) == int((np.asarray(back) != value).sum()), "the padding is not empty"


# ---- the relations: fn has the public function's meaning, numpy in and numpy out ----------------------------
def relate_labelling(fn, aff, base, t, off=0.0):
    """fn(aff) -> labels numbered by first voxel: the same partition and K; the same array where order is kept."""
    out = fn(t.affinities(aff, 1.0, off))
    back = t.back(out)
    _same_outside(out, back)
    assert same_labelling(back, base), t.name
    if t.keeps_order:
        np.testing.assert_array_equal(back, base, err_msg=t.name)
    return out


def relate_region_graph(fn, frags_t, aff, base_frags, base_graph, t, off=0.0):
    """fn(labels, aff) -> (edges, counts, sums, sizes) on the transformed fragments frags_t."""
    table = correspondence(t.back(frags_t), base_frags)
    edges, counts, sums, sizes = fn(frags_t, t.affinities(aff, 1.0, off))
    b_edges, b_counts, b_sums, b_sizes = base_graph
    assert graph_dict(edges, counts, sums, table) == graph_dict(b_edges, b_counts, b_sums), t.name
    assert len(sizes) == len(b_sizes) and sizes[0] == b_sizes[0] + t.padding, t.name
    np.testing.assert_array_equal(sizes[1:], np.asarray(b_sizes)[table[1:]], err_msg=t.name)


def relate_fill_holes(fn, labels, base, t):
    """fn(labels) -> (filled, n_holes, n_voxels)."""
    out, n_holes, n_voxels = fn(t.volume(labels))
    back = t.back(out)
    _same_outside(out, back)
    np.testing.assert_array_equal(back, base[0], err_msg=t.name)
    assert (n_holes, n_voxels) == (base[1], base[2]), t.name


def relate_dbf(fn, labels, base, t, border):
    """fn(labels, black_border) -> field, under a symmetry."""
    np.testing.assert_array_equal(t.back(fn(t.volume(labels), border)), base, err_msg=f"{t.name} border={border}")


def relate_dbf_padding(fn, labels, base_black, t):
    """Under a translation the padding is background, which bounds every label: the black-border field is
    kept as it is, and with at least one voxel of padding on every side the plain field equals it too."""
    padded = t.volume(labels)
    out = fn(padded, True)
    back = t.back(out)
    _same_outside(out, back)
    np.testing.assert_array_equal(back, base_black, err_msg=t.name)
    if min(t.offset) >= 1 and min(t.tail) >= 1:
        out = fn(padded, False)
        back = t.back(out)
        _same_outside(out, back)
        np.testing.assert_array_equal(back, base_black, err_msg=f"{t.name}, no border")
        return 2
    return 1


def relate_segment_table(fn, labels, dbf, base, t):
    """fn(labels, dbf) -> (sizes, boxes, peak, peak_index) with K + 1 rows."""
    sizes, boxes, peak, peak_index = fn(t.volume(labels), t.volume(dbf))
    b_sizes, b_boxes, b_peak, b_index = base
    assert sizes[0] == b_sizes[0] + t.padding, t.name
    np.testing.assert_array_equal(sizes[1:], b_sizes[1:], err_msg=t.name)
    np.testing.assert_array_equal(peak, b_peak, err_msg=t.name)
    np.testing.assert_array_equal(boxes, t.boxes(b_boxes), err_msg=t.name)
    back = t.back_indices(peak_index)
    np.testing.assert_array_equal(back < 0, b_index < 0, err_msg=t.name)
    rows = np.flatnonzero(back >= 0)
    np.testing.assert_array_equal(np.asarray(labels).reshape(-1)[back[rows]], rows, err_msg=t.name)
    np.testing.assert_array_equal(np.asarray(dbf).reshape(-1)[back[rows]], b_peak[rows], err_msg=t.name)
    if t.keeps_order:
        np.testing.assert_array_equal(back, b_index, err_msg=t.name)


def relate_pieces(fn, labels, dust, base, t):
    """fn(labels, dust) -> (pieces, piece_label, piece_size, piece_first). The number of kept pieces is
    the same, and so is the dust count, every piece less the kept ones."""
    pieces, piece_label, piece_size, piece_first = fn(t.volume(labels), dust)
    b_pieces, b_label, b_size, b_first = base
    back = t.back(pieces)
    _same_outside(pieces, back)
    assert same_labelling(back, b_pieces) and len(piece_label) == len(b_label), t.name
    table = correspondence(back, b_pieces)[1:] - 1      # row of this run -> row of the baseline
    np.testing.assert_array_equal(piece_label, b_label[table], err_msg=t.name)
    np.testing.assert_array_equal(piece_size, b_size[table], err_msg=t.name)
    flat = pieces.reshape(-1)      # piece_first is each piece's smallest index in the volume it was given
    first = np.full(len(piece_label) + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    np.testing.assert_array_equal(piece_first, first[1:], err_msg=t.name)
    if t.keeps_order:
        np.testing.assert_array_equal(back, b_pieces, err_msg=t.name)
        np.testing.assert_array_equal(t.back_indices(piece_first), b_first, err_msg=t.name)


def relate_geodesic(fn, labels, sources, cost, base, t):
    """fn(labels, sources, cost) -> (field, far_value, far_index)."""
    field, far_value, far_index = fn(t.volume(labels), t.indices(sources),
                                     None if cost is None else t.volume(cost, np.float32(1.0)))
    b_field, b_value, b_index = base
    back = t.back(field)
    assert int((bits(field) != 0).sum()) == int((bits(back) != 0).sum()), "the padding is not +0.0"
    np.testing.assert_array_equal(bits(back), bits(b_field), err_msg=t.name)
    np.testing.assert_array_equal(bits(far_value), bits(b_value), err_msg=t.name)
    at = t.back_indices(far_index)
    np.testing.assert_array_equal(at < 0, b_index < 0, err_msg=t.name)
    rows = np.flatnonzero(at >= 0)
    np.testing.assert_array_equal(np.asarray(labels).reshape(-1)[at[rows]], rows, err_msg=t.name)
    np.testing.assert_array_equal(bits(b_field).reshape(-1)[at[rows]], bits(b_value)[rows], err_msg=t.name)
    if t.keeps_order:
        np.testing.assert_array_equal(at, b_index, err_msg=t.name)


# ---- the relations under a renaming of the labels: table[L] is the new name of L ----------------------------
def rename_dbf(fn, labels, base, table, border):
    np.testing.assert_array_equal(fn(relabel_volume(labels, table), border), base)


def rename_fill_holes(fn, labels, base, table):
    out, n_holes, n_voxels = fn(relabel_volume(labels, table))
    np.testing.assert_array_equal(out, relabel_volume(base[0], table))
    assert (n_holes, n_voxels) == (base[1], base[2])


def rename_segment_table(fn, labels, dbf, base, table):
    got = fn(relabel_volume(labels, table), dbf)
    for g, b, absent in zip(got, base, (0, 0, 0, -1)):
        np.testing.assert_array_equal(g, relabel_rows(b, table, absent))


def rename_region_graph(fn, labels, aff, base, table):
    edges, counts, sums, sizes = fn(relabel_volume(labels, table), aff)
    b_edges, b_counts, b_sums = relabel_edges(base[0], table, base[1], base[2])
    np.testing.assert_array_equal(edges, b_edges)
    np.testing.assert_array_equal(counts, b_counts)
    np.testing.assert_array_equal(sums, b_sums)
    np.testing.assert_array_equal(sizes, relabel_rows(base[3], table, 0))


def rename_pieces(fn, labels, dust, base, table):
    """Numbering by first voxel does not look at the names: the pieces are the same array."""
    pieces, piece_label, piece_size, piece_first = fn(relabel_volume(labels, table), dust)
    np.testing.assert_array_equal(pieces, base[0])
    np.testing.assert_array_equal(piece_label, np.asarray(table)[base[1]])
    np.testing.assert_array_equal(piece_size, base[2])
    np.testing.assert_array_equal(piece_first, base[3])


def rename_geodesic(fn, labels, sources, cost, base, table):
    field, far_value, far_index = fn(relabel_volume(labels, table), relabel_rows(sources, table, -1), cost)
    np.testing.assert_array_equal(bits(field), bits(base[0]))
    np.testing.assert_array_equal(bits(far_value), bits(relabel_rows(base[1], table, 0)))
    np.testing.assert_array_equal(far_index, relabel_rows(base[2], table, -1))


# ---- one base volume with everything the relations need, checked before anything runs on it ----------------
WATERSHED_THRESHOLDS = [(0.1, 0.9999), (0.3, 0.7)]      # the default pair, and one with high inside the values
MIN_SIZES = (0, 5)                                      # nothing dropped, and a size filter that drops some
_BASES = {}


def affinity_inputs(shape, seed=0, spans_tiles=True):
    """watershed (tie-free affinities), components (affinities near percolation) and threshold of one shape,
    each asserted to be a case worth running."""
    import watershed_ref

    watershed = watershed_affinities(shape, seed + 11)
    for low, high in WATERSHED_THRESHOLDS:
        assert watershed_ref.tied_voxels(watershed, low, high) == 0
        frags, count = watershed_ref.fragments(watershed, low, high, 0)
        assert count > 1
        above_low = np.nextafter(np.float32(low), np.float32(np.inf))      # tests/test_watershed_cpu.py's guard
        assert not np.array_equal(frags, components_ref.components(watershed, above_low, 0)[0])
        assert not np.array_equal(frags, components_ref.components(watershed, high, 0)[0])
    assert watershed.min() <= WATERSHED_THRESHOLDS[1][1] <= watershed[watershed < 1].max()

    components, threshold = component_affinities(shape, seed + 3)
    whole, count = components_ref.components(components, threshold, MIN_SIZES[0])
    _, fewer = components_ref.components(components, threshold, MIN_SIZES[1])
    assert 1 <= fewer < count      # the size filter drops some and keeps some
    if spans_tiles:
        assert tiles_of_largest(whole) >= 3
    half = components.astype(np.float16)
    # float16 is a case of its own
    assert not np.array_equal(components_ref.components(half, threshold, 0)[0], whole)

    return dict(watershed=watershed, components=components, threshold=threshold)


def stream_inputs(shape=(19, 11, 45), seed=0):
    """The affinities of the streamed relations: three slabs at a depth of 8, four at a depth of 5."""
    key = ("stream", tuple(shape), seed)
    if key not in _BASES:
        _BASES[key] = dict(shape=tuple(shape), **affinity_inputs(shape, seed))
    return _BASES[key]


def base_inputs(shape, seed=0, dust=DUST, spans_tiles=True, **label_options):
    """
    A dict of read-only inputs of one shape, each asserted to have what makes the relations worth running:
    labels, k, sources, cost, dust, facts; watershed (affinities); components (affinities), threshold.
    spans_tiles=False is for volumes smaller than a tile, where only the tile conditions are left out.
    """
    import geodesic_ref

    key = (tuple(shape), seed, dust, spans_tiles, tuple(sorted(label_options.items())))
    if key in _BASES:
        return _BASES[key]
    rng = np.random.default_rng(seed)
    labels = label_volume(shape, seed, **label_options)
    k = int(labels.max())
    sources = geodesic_ref.random_sources(rng, labels, k)
    cost = geodesic_ref.random_cost(rng, shape)
    facts = label_facts(labels, sources, dust)
    assert facts["k"] >= 8 and (sources[1:] >= 0).all(), facts
    assert facts["touching_faces"] >= 1 and facts["holes"] >= 1 and facts["hole_voxels"] >= 1, facts
    assert facts["split_labels_with_dust"] >= 1 and facts["dust_pieces"] >= 1 and facts["kept_pieces"] >= 1, facts
    assert facts["unreachable"] >= 1, facts
    if spans_tiles:
        assert all(n % t and n > t for n, t in zip(shape, TILE)) and len(set(shape)) == 3, shape
        assert facts["tiles_spanned"] >= 2, facts
    inside = cost[labels > 0]
    with np.errstate(invalid="ignore"):
        assert (inside == 0).any() and np.isposinf(inside).any() and (inside < 0).any() and np.isnan(inside).any()
    cost.setflags(write=False)
    sources.setflags(write=False)

    base = dict(shape=tuple(shape), labels=labels, k=k, sources=sources, cost=cost, dust=dust, facts=facts,
                **affinity_inputs(shape, seed, spans_tiles))
    _BASES[key] = base
    return base
