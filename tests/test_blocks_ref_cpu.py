"""
The block grid, the ownership rule and join_block_skeletons without a GPU, against tests/blocks_ref.py: the grid at
n = 1, n <= b, n = k (b - 1) + 1 and with a thin last block of two planes; every voxel is owned exactly once;
join_block_skeletons equals the reference join, which searches a graph and has no union-find, on hand-made trees (a
chain of three blocks, a ring, four trees at one voxel, dust by summed owned size at t - 1 and t, seeded random
forests); the order of the records does not matter; and the refusals.
"""

import itertools

import numpy as np
import pytest

import blocks_ref
from aind_exaspim_neuron_segmentation_amd import segmentation


@pytest.mark.parametrize("n, b, want", [
    (1, 2, [(0, 1)]), (1, 512, [(0, 1)]), (2, 2, [(0, 2)]), (5, 5, [(0, 5)]), (5, 9, [(0, 5)]),
    (3, 2, [(0, 2), (1, 3)]), (9, 5, [(0, 5), (4, 9)]), (13, 5, [(0, 5), (4, 9), (8, 13)]),
    (6, 5, [(0, 5), (4, 6)]), (10, 5, [(0, 5), (4, 9), (8, 10)]), (7, 3, [(0, 3), (2, 5), (4, 7)]),
])
def test_the_spans_of_an_axis(n, b, want):
    assert blocks_ref.spans(n, b) == want
    assert segmentation._block_spans(n, b) == want
    for (_, end), (start, _) in zip(want, want[1:]):
        assert end - start == 1      # exactly one shared plane
    assert all(end - start >= 2 for start, end in want) or n == 1
    assert want[-1][1] == n


def test_every_length_and_block_length():
    for n, b in itertools.product(range(1, 40), range(2, 12)):
        assert segmentation._block_spans(n, b) == blocks_ref.spans(n, b), (n, b)


@pytest.mark.parametrize("shape, block", [((1, 1, 1), (2, 2, 2)), ((5, 6, 7), (9, 9, 9)), ((9, 9, 9), (5, 5, 5)),
                                          ((6, 10, 13), (5, 5, 5)), ((1, 7, 8), (4, 3, 2)), ((12, 11, 10), (4, 11, 6))])
def test_every_voxel_is_owned_exactly_once(shape, block):
    owners = np.zeros(shape, dtype=np.int32)
    covered = np.zeros(shape, dtype=np.int32)
    blocks = blocks_ref.grid(shape, block)
    for b in blocks:
        (z0, y0, x0), (z1, y1, x1) = b["lo"], b["hi"]
        size = (z1 - z0, y1 - y0, x1 - x0)
        high = [False, b["open"][1], False, b["open"][3], False, b["open"][5]]
        owners[z0:z1, y0:y1, x0:x1] += ~blocks_ref.face_mask(size, high)
        covered[z0:z1, y0:y1, x0:x1] += 1
        ones = np.ones(size, dtype=np.int32)
        assert blocks_ref.owned_sizes(ones, 1, b["open"])[0] == np.count_nonzero(~blocks_ref.face_mask(size, high))
    assert (owners == 1).all() and (covered >= 1).all()
    assert blocks[0]["open"][::2] == [False] * 3 and blocks[-1]["open"][1::2] == [False] * 3
    assert len(blocks) == np.prod([len(blocks_ref.spans(n, b)) for n, b in zip(shape, block)])


def test_the_open_rule_of_the_reference():
    labels = np.zeros((4, 5, 6), dtype=np.int32)
    labels[0, 0, 0:2] = 1      # 2 voxels on z = 0, y = 0 and x = 0
    labels[2, 2, 2:5] = 1      # 3 voxels inside
    labels[3, 4, 5] = 2      # 1 voxel on z = D - 1, y = H - 1, x = W - 1
    closed = blocks_ref.open_pieces(labels, 2, 3, [False] * 6)
    assert closed[1].tolist() == [1] and closed[5:] == (2, 0)
    low = blocks_ref.open_pieces(labels, 2, 3, [True, False, False, False, False, False])
    assert low[1].tolist() == [1, 1] and low[4].tolist() == [True, False] and low[5:] == (1, 1)
    high = blocks_ref.open_pieces(labels, 2, 3, [False, False, False, False, False, True])
    assert high[1].tolist() == [1, 2] and high[4].tolist() == [False, True] and high[5:] == (1, 1)
    assert high[0][3, 4, 5] == 2 and high[0][0, 0, 0] == 0


def line(x0, x1, y=0, z=0):
    step = 1 if x1 >= x0 else -1
    return [(z, y, x) for x in range(x0, x1 + step, step)]


def same(got, want):
    assert list(got) == list(want)
    for label in want:
        for a, b in zip(got[label], want[label]):
            assert a.dtype == b.dtype and a.shape == b.shape, label
            np.testing.assert_array_equal(a, b)


def held(trees, dust=0):
    stats = {}
    got = segmentation.join_block_skeletons(trees, dust, stats)
    want, joints, skipped, dusty = blocks_ref.join(trees, dust)
    same(got, want)
    assert (stats["joints"], stats["skipped_joints"], stats["dust_components"]) == (joints, skipped, dusty)
    assert stats["trees"] == len(trees) and stats["join_seconds"] >= 0
    for vertices, parent, radius in got.values():
        assert vertices.dtype == np.int32 and parent.dtype == np.int32 and radius.dtype == np.float32
        step = np.abs(vertices[parent[parent >= 0]] - vertices[parent >= 0]).max(axis=1, initial=0)
        assert (step <= 1).all()      # the hand-made trees keep child and parent 26-adjacent through a join
    return got, stats


def chain_of_three():
    """Blocks cut at x = 4 and x = 8; the middle tree is rooted in its middle, so it has to be re-oriented."""
    a = blocks_ref.path_tree(0, 1, 7, line(0, 4), 4, [4], radius=[1, 1, 1, 1, 3])
    middle = line(6, 4) + line(7, 8)
    b = blocks_ref.path_tree(1, 1, 7, middle, 4, [2, 4], radius=[1, 1, 2, 1, 2])
    b["parent"] = np.array([-1, 0, 1, 0, 3], dtype=np.int32)
    c = blocks_ref.path_tree(2, 2, 7, line(12, 8), 5, [4], radius=[1, 1, 1, 1, 5])
    return [a, b, c]


def test_a_chain_of_three_blocks():
    got, stats = held(chain_of_three())
    vertices, parent, radius = got[7]
    assert (stats["joints"], stats["skipped_joints"]) == (2, 0)
    assert len(parent) == 5 + 5 + 5 - 2 and np.count_nonzero(parent == -1) == 1 and parent[0] == -1
    assert sorted(vertices[:, 2].tolist()) == list(range(13))
    assert radius[vertices[:, 2] == 4] == 2 and radius[vertices[:, 2] == 8] == 2      # the smaller of the two
    order = np.argsort(vertices[:, 2])      # rooted at x = 0: every parent is the vertex one step to the left
    assert (vertices[parent[order[1:]], 2] == vertices[order[1:], 2] - 1).all()


def ring(block=0):
    """Two trees that meet at (0, 0, 4) and at (0, 2, 4): the second meeting would close a ring."""
    a = blocks_ref.path_tree(block, 1, 3, line(4, 2, y=0) + [(0, 1, 1)] + line(2, 4, y=2), 6, [0, 6])
    b = blocks_ref.path_tree(block + 1, 1, 3, line(4, 6, y=0) + [(0, 1, 7)] + line(6, 4, y=2), 6, [0, 6])
    return [a, b]


def test_a_ring_keeps_one_duplicate_vertex():
    got, stats = held(ring())
    vertices, parent, _ = got[3]
    assert (stats["joints"], stats["skipped_joints"]) == (2, 1)
    assert len(parent) == 7 + 7 - 1 and np.count_nonzero(parent == -1) == 1
    assert np.count_nonzero((vertices == (0, 2, 4)).all(axis=1)) == 2
    assert np.count_nonzero((vertices == (0, 0, 4)).all(axis=1)) == 1


def four_at_one_voxel():
    """The corner of a 2 x 2 grid in (y, x): four trees of one label end at (0, 4, 4), one of another label too."""
    ends = [(0, 0, 0), (0, 0, 8), (0, 8, 0), (0, 8, 8)]
    trees = []
    for block, (z, y, x) in enumerate(ends):
        voxels = [(0, y + (i if y == 0 else -i), x + (i if x == 0 else -i)) for i in range(5)]
        trees.append(blocks_ref.path_tree(block, 1, 2, voxels, 4, [4], radius=[1, 1, 1, 1, 9 - block]))
    trees.append(blocks_ref.path_tree(3, 2, 5, [(1, 4, 4), (0, 4, 4)], 2, [1]))
    return trees


def test_four_trees_meet_at_one_voxel():
    got, stats = held(four_at_one_voxel())
    assert (stats["joints"], stats["skipped_joints"]) == (1, 0) and list(got) == [2, 5]
    vertices, parent, radius = got[2]
    assert len(parent) == 4 * 5 - 3 and np.count_nonzero(parent == -1) == 1
    centre = np.nonzero((vertices == (0, 4, 4)).all(axis=1))[0]
    assert len(centre) == 1 and radius[centre[0]] == 6 and np.count_nonzero(parent == centre[0]) == 3
    assert len(got[5][1]) == 2


def test_dust_is_judged_by_the_summed_owned_size():
    trees = chain_of_three() + [blocks_ref.path_tree(1, 2, 7, line(0, 2, y=5), 3, [])]
    total = 4 + 4 + 5
    for dust, kept in ((0, 2), (3, 2), (4, 1), (total - 1, 1), (total, 1), (total + 1, 0)):
        got, stats = held(trees, dust)
        assert stats["dust_components"] == 2 - kept
        assert (np.count_nonzero(got[7][1] == -1) if kept else len(got)) == kept


def test_a_label_in_two_components_and_a_lone_vertex():
    trees = chain_of_three() + [blocks_ref.path_tree(0, 2, 7, [(3, 3, 3)], 1, []),
                                blocks_ref.path_tree(2, 1, 4, line(9, 11, y=4), 3, [0])]
    got, _ = held(trees)
    assert list(got) == [7, 4] and np.count_nonzero(got[7][1] == -1) == 2
    assert got[7][0][13].tolist() == [3, 3, 3] and got[7][1][13] == -1      # the second component, after the first
    assert held([])[0] == {}


def random_forest(seed):
    """Random walks in a 2 x 2 grid of blocks that end on the shared planes: joints, rings and lone trees."""
    rng = np.random.default_rng(seed)
    trees = []
    meeting = sorted({(0, 4, int(x)) for x in rng.integers(0, 9, 3)} | {(0, int(y), 4) for y in rng.integers(0, 9, 3)})
    for block in range(4):
        for piece in range(1, int(rng.integers(2, 5))):
            ends = [meeting[i] for i in rng.choice(len(meeting), size=int(rng.integers(0, 3)), replace=False)]
            voxels = [(1 + block, piece, i) for i in range(int(rng.integers(1, 4)))]
            rows = list(range(len(voxels), len(voxels) + len(ends)))
            tree = blocks_ref.path_tree(block, piece, int(rng.integers(1, 3)), voxels + ends,
                                        int(rng.integers(0, 6)), rows, radius=rng.integers(1, 9, len(voxels + ends)))
            tree["parent"][len(voxels):] = int(rng.integers(0, len(voxels)))      # a star, not a chain
            trees.append(tree)
    return trees


@pytest.mark.parametrize("seed", range(12))
def test_random_forests_and_the_order_of_the_records(seed):
    trees = random_forest(seed)
    stats = {}
    want = segmentation.join_block_skeletons(trees, 4, stats)
    reference, joints, skipped, dusty = blocks_ref.join(trees, 4)
    same(want, reference)
    assert (stats["joints"], stats["skipped_joints"], stats["dust_components"]) == (joints, skipped, dusty)
    rng = np.random.default_rng(100 + seed)
    for _ in range(3):
        shuffled = [trees[i] for i in rng.permutation(len(trees))]
        same(segmentation.join_block_skeletons(shuffled, 4), want)


def test_the_random_forests_hold_joints_skips_and_dust():
    totals = np.zeros(3, dtype=np.int64)
    for seed in range(12):
        totals += blocks_ref.join(random_forest(seed), 4)[1:]
    assert (totals > 0).all(), totals


def test_the_output_goes_through_the_writers():
    got, _ = held(chain_of_three() + ring(5))
    assert segmentation.voxelize_skeletons(got, (1, 3, 13)).max() == 7
    for skeleton in got.values():
        assert len(segmentation.skeleton_to_swc(*skeleton).splitlines()) >= len(skeleton[1])


def test_refusals():
    join = segmentation.join_block_skeletons
    good = chain_of_three()
    with pytest.raises(TypeError, match="trees must be a list"):
        join({})
    with pytest.raises(TypeError, match="record 0 must be a dict"):
        join([(1, 2)])
    with pytest.raises(TypeError, match="dust_threshold must be an integer"):
        join(good, 1.5)
    with pytest.raises(ValueError, match="dust_threshold must not be negative"):
        join(good, -1)
    with pytest.raises(TypeError, match="stats must be a dict"):
        join(good, 0, [])

    def broken(**changes):
        return [dict(good[0], **changes)] + good[1:]

    lacking = dict(good[0])
    del lacking["owned_size"]
    with pytest.raises(ValueError, match="lacks owned_size"):
        join([lacking])
    with pytest.raises(TypeError, match="block must be an integer"):
        join(broken(block=0.0))
    with pytest.raises(ValueError, match="piece must be at least 1"):
        join(broken(piece=0))
    with pytest.raises(ValueError, match="owned_size must not be negative"):
        join(broken(owned_size=-1))
    with pytest.raises(ValueError, match=r"vertices \(n, 3\)"):
        join(broken(vertices=good[0]["vertices"][:-1]))
    with pytest.raises(ValueError, match=r"vertices \(n, 3\)"):
        join(broken(radius=good[0]["radius"][:-1]))
    with pytest.raises(TypeError, match="must be integers"):
        join(broken(vertices=good[0]["vertices"].astype(np.float32)))
    with pytest.raises(ValueError, match="negative coordinate"):
        join(broken(vertices=good[0]["vertices"] - 1))
    with pytest.raises(ValueError, match="one -1"):
        join(broken(parent=np.array([-1, 0, 1, -1, 3])))
    with pytest.raises(ValueError, match="one -1"):
        join(broken(parent=np.array([-1, 0, 1, 2, 5])))
    with pytest.raises(ValueError, match="border_rows must be distinct rows"):
        join(broken(border_rows=np.array([5])))
    with pytest.raises(ValueError, match="border_rows must be distinct rows"):
        join(broken(border_rows=np.array([4, 4])))
    with pytest.raises(ValueError, match="two records for piece 1 of block 0"):
        join(good + [good[0]])
    with pytest.raises(RuntimeError, match="not connected"):
        join(broken(parent=np.array([-1, 0, 1, 4, 3])))      # a cycle that the root does not reach
