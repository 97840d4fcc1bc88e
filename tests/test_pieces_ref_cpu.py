"""
The two host oracles of label_pieces against each other (no GPU): the flood fill over the 26 neighbours and the
per-label scipy labelling give the same volume, tables and dust count on seeded volumes of sides 3 .. 14 and on the
crafted cases (tile-seam pairs, checkerboards, separated pieces, the snake, the label range, dust), and the two
consequences DESIGN 6q proves hold against tests/dbf_ref.py and tests/border_ref.py: the distance-to-boundary
field of the pieces is that of the labels on every kept piece, and the border targets of the pieces are those of
the labels restricted to kept pieces, with the label column mapped to piece numbers.
"""

import numpy as np
import pytest

import border_ref
import dbf_ref
import pieces_ref

CRAFTED = pieces_ref.crafted()


def same(a, b):
    assert len(a) == len(b) == 5
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
    assert a[4] == b[4]


def seeded(seed):
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(int(v) for v in rng.integers(3, 15, size=3))
    return pieces_ref.random_volume(seed, shape), int(rng.integers(0, 7))


@pytest.mark.parametrize("seed", range(40))
def test_the_oracles_agree_on_seeded_volumes(seed):
    labels, dust = seeded(seed)
    for k in (3, 2):
        a = pieces_ref.flood_fill(labels, k, dust)
        same(a, pieces_ref.by_label(labels, k, dust))
        pieces, piece_label, piece_size, piece_first, _ = a
        # the tables are what the volume says
        assert (np.diff(piece_first) > 0).all() and (piece_size >= max(dust, 1)).all()
        for number, (label, size, first) in enumerate(zip(piece_label, piece_size, piece_first), start=1):
            mine = np.flatnonzero(pieces.reshape(-1) == number)
            assert len(mine) == size and mine[0] == first and (labels.reshape(-1)[mine] == label).all()
        assert not pieces[(labels < 1) | (labels > k)].any()


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_the_oracles_agree_on_the_crafted_cases(name):
    labels, k, dust, kept = CRAFTED[name]
    a = pieces_ref.flood_fill(labels, k, dust)
    same(a, pieces_ref.by_label(labels, k, dust))
    if kept is not None:
        assert len(a[1]) == kept == int(a[0].max())


def test_the_dust_counts():
    labels = pieces_ref.dust_volume(4)
    assert [pieces_ref.flood_fill(labels, 1, t)[4] for t in (0, 1, 3, 4, 5, 6)] == [0, 0, 0, 1, 2, 3]
    assert pieces_ref.flood_fill(labels, 1, 5)[2].tolist() == [5]


def mapped_targets(labels, k, pieces):
    """border_ref's targets of the labels, restricted to kept pieces, the label column mapped to piece numbers."""
    rows = border_ref.by_component(labels, k)
    number = pieces.reshape(-1)[rows[:, 1]]
    rows = np.stack([number[number > 0].astype(np.int64), rows[number > 0, 1]], axis=1)
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))].reshape(-1, 2)


@pytest.mark.parametrize("seed", range(12))
def test_the_two_consequences(seed):
    labels, dust = seeded(seed)
    k = 3
    pieces, piece_label, _, _, _ = pieces_ref.flood_fill(labels, k, dust)
    fg = pieces_ref.foreground(labels, k).astype(np.int32)      # the field of the labels the pieces are taken of
    # (a) the field, with and without the black border
    for border in (False, True):
        want = dbf_ref.brute_force(fg, border)
        got = dbf_ref.brute_force(pieces, border)
        np.testing.assert_array_equal(got[pieces > 0], want[pieces > 0])
    # (b) the border targets
    np.testing.assert_array_equal(border_ref.by_component(pieces, len(piece_label)), mapped_targets(fg, k, pieces))
