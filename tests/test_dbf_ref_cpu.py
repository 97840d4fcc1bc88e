"""
The two oracles of the distance-to-boundary field (tests/dbf_ref.py) agree exactly -- brute force over
all voxel pairs and the per-label scipy EDT read through its integer indices -- on seeded volumes of
side 1 .. 14 in both border modes, on the degenerate volumes by name, and on hand-built rows along each
axis whose values are written out. The oracle composed of small blocks between zero rows (tiled_rows, for
the volumes of 10^7 voxels of tests/test_gpu_dbf.py) is held to per_label of the whole composed volume.
The numpy segment table is held to a loop over the voxels.
"""

import numpy as np
import pytest

import dbf_ref
from dbf_ref import DBF_INF

MODES = [False, True]


def random_volume(seed):
    rng = np.random.default_rng(seed)
    shape = tuple(int(v) for v in rng.integers(1, 15, size=3))
    kind = seed % 4
    if kind == 0:
        labels = rng.integers(0, 4, size=shape)                      # noise: touching labels and background
    elif kind == 1:
        labels = dbf_ref.stretched_labels(rng, shape, top=3, longest=9)
    elif kind == 2:
        labels = rng.integers(1, 3, size=shape)                      # no background at all
    else:
        labels = rng.integers(-2, 3, size=shape) * rng.integers(0, 2, size=shape)   # negative labels, sparse
    return labels.astype(np.int32)


@pytest.mark.parametrize("seed", range(44))
def test_brute_force_and_scipy_agree_on_seeded_volumes(seed):
    labels = random_volume(seed)
    for border in MODES:
        want = dbf_ref.brute_force(labels, border)
        got = dbf_ref.per_label(labels, border)
        assert got.dtype == want.dtype == np.int32
        np.testing.assert_array_equal(got, want)
        assert (want[labels <= 0] == 0).all() and (want[labels > 0] >= 1).all()


def named_volumes():
    checker = (np.indices((6, 5, 7)).sum(axis=0) % 2 + 1).astype(np.int32)
    halves = np.ones((5, 6, 8), dtype=np.int32)
    halves[:, :, 4:] = 2
    negative = np.full((4, 5, 6), -3, dtype=np.int32)
    negative[1:3, 1:4, 2:5] = 7
    big = np.full((3, 4, 5), 2**31 - 1, dtype=np.int32)
    big[1, 2, 2] = -(2**31)
    return {
        "all background": np.zeros((4, 5, 6), dtype=np.int32),
        "one label everywhere": np.full((5, 4, 7), 3, dtype=np.int32),
        "checkerboard": checker,
        "touching halves": halves,
        "negative labels": negative,
        "extreme values": big,
        "one voxel": np.ones((1, 1, 1), dtype=np.int32),
        "one background voxel": np.zeros((1, 1, 1), dtype=np.int32),
    }


@pytest.mark.parametrize("name", list(named_volumes()))
def test_named_volumes(name):
    labels = named_volumes()[name]
    got = {}
    for border in MODES:
        got[border] = dbf_ref.brute_force(labels, border)
        np.testing.assert_array_equal(dbf_ref.per_label(labels, border), got[border])
    if name == "all background":
        assert not got[False].any() and not got[True].any()
    if name == "one label everywhere":
        assert (got[False] == DBF_INF).all()
        z, y, x = np.indices(labels.shape)
        d, h, w = labels.shape
        face = np.minimum.reduce([z + 1, d - z, y + 1, h - y, x + 1, w - x])
        np.testing.assert_array_equal(got[True], face ** 2)
    if name == "checkerboard":
        assert (got[False] == 1).all() and (got[True] == 1).all()
    if name == "touching halves":
        x = np.indices(labels.shape)[2]
        np.testing.assert_array_equal(got[False], np.where(x < 4, 4 - x, x - 3) ** 2)
    if name == "one voxel":
        assert got[False].item() == DBF_INF and got[True].item() == 1


ROW = np.array([0, 1, 1, 1, 1, 1, 2, 2, 0, 3, 3, 3], dtype=np.int32)
ROW_OPEN = np.array([0, 1, 4, 9, 4, 1, 1, 1, 0, 1, 4, 9], dtype=np.int64)   # the face bounds nothing
ROW_BORDER = np.array([0, 1, 4, 9, 4, 1, 1, 1, 0, 1, 4, 1], dtype=np.int64)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_hand_built_rows(axis):
    shape = [1, 1, 1]
    shape[axis] = ROW.size
    labels = ROW.reshape(shape)
    # a single row: without the border the last run has a boundary on one side only
    open_row = ROW_OPEN
    for fn in (dbf_ref.brute_force, dbf_ref.per_label):
        np.testing.assert_array_equal(fn(labels, False).reshape(-1), open_row)
        # with the border the two unit axes bound every voxel at distance 1
        np.testing.assert_array_equal(fn(labels, True).reshape(-1), np.minimum(ROW_BORDER, 1))
    # three rows side by side along another axis, the same labels: the unit distance to the border across
    wide = [3, 3, 3]
    wide[axis] = ROW.size
    block = np.broadcast_to(labels, wide)
    for fn in (dbf_ref.brute_force, dbf_ref.per_label):
        got = fn(block, False)
        np.testing.assert_array_equal(np.moveaxis(got, axis, 2)[1, 1], open_row)
        got = fn(block, True)
        np.testing.assert_array_equal(np.moveaxis(got, axis, 2)[1, 1], np.minimum(ROW_BORDER, 4))
        np.testing.assert_array_equal(np.moveaxis(got, axis, 2)[0, 1], np.minimum(ROW_BORDER, 1))


def test_a_diagonal_neighbour_is_found():
    labels = np.ones((5, 5, 5), dtype=np.int32)
    labels[0, 0, 0] = 0
    want = (np.indices(labels.shape) ** 2).sum(axis=0)
    for fn in (dbf_ref.brute_force, dbf_ref.per_label):
        np.testing.assert_array_equal(fn(labels, False), want)


@pytest.mark.parametrize("border", MODES)
def test_tiled_rows_equal_per_label_of_the_whole_volume(border):
    rng = np.random.default_rng(53)
    shape = (3, 11, 70)
    blocks = [dbf_ref.stretched_labels(rng, shape, top=3, longest=90) for _ in range(4)]
    blocks.append(np.full(shape, 2, dtype=np.int32))                 # one label throughout: bounded by the zero rows
    choice = [4, 0, 1, 4, 4, 2, 3, 0, 2]                             # the solid block first, and twice in a row
    labels, expected = dbf_ref.tiled_rows(blocks, choice, border)
    assert labels.shape == expected.shape == (3, 1 + 12 * len(choice), 70)
    assert labels.dtype == expected.dtype == np.int32 and labels.flags.c_contiguous
    assert not labels[:, ::12].any() and not expected[:, ::12].any()
    for i, c in enumerate(choice):
        np.testing.assert_array_equal(labels[:, 1 + 12 * i:12 + 12 * i], blocks[c])
    np.testing.assert_array_equal(expected, dbf_ref.per_label(labels, border))
    solid = expected[:, 1:12]                                         # the first block is the solid one
    assert solid.max() == (36 if not border else 4)                   # 6 rows to a zero row; 2 planes to a z face


def test_segment_table_against_a_loop():
    rng = np.random.default_rng(3)
    labels = rng.integers(-1, 7, size=(5, 6, 7)).astype(np.int32)
    labels[labels == 4] = 0                                          # an absent id below the maximum
    dbf = rng.integers(0, 5, size=labels.shape).astype(np.int32)     # many ties
    for field in (None, dbf):
        for k in (6, 3, 0, 9):
            sizes, boxes, peak, index = dbf_ref.segment_table(labels, field, k)
            assert sizes.shape == peak.shape == index.shape == (k + 1,) and boxes.shape == (k + 1, 6)
            assert sizes[0] == (labels == 0).sum() and not boxes[0].any() and peak[0] == 0 and index[0] == -1
            for lab in range(1, k + 1):
                where = np.argwhere(labels == lab)
                assert sizes[lab] == len(where)
                if len(where) == 0:
                    assert not boxes[lab].any() and peak[lab] == 0 and index[lab] == -1
                    continue
                assert list(boxes[lab]) == list(where.min(axis=0)) + list(where.max(axis=0) + 1)
                flat = np.flatnonzero(labels.reshape(-1) == lab)
                values = np.zeros(flat.size, dtype=np.int64) if field is None else field.reshape(-1)[flat]
                assert peak[lab] == values.max()
                assert index[lab] == flat[values == values.max()][0]
            for a, b in zip(dbf_ref.segment_table_sorted(labels, field, k), (sizes, boxes, peak, index)):
                assert a.dtype == b.dtype
                np.testing.assert_array_equal(a, b)
    sizes = dbf_ref.segment_table(labels)[0]
    assert sizes.shape == (7,)
    empty = np.full((2, 3, 4), -1, dtype=np.int32)
    for a, b in zip(dbf_ref.segment_table_sorted(empty, None, 2), dbf_ref.segment_table(empty, None, 2)):
        np.testing.assert_array_equal(a, b)
