"""
inference.skeletonize_blocks on the GPU (-m gpu), at the small scale and const of the neighbouring tests, on volumes
of a few thousand voxels. DESIGN 6r's four properties: (a) with one block it is skeletonize_pieces(fix_borders=True)
array for array, on the volumes of test_gpu_skeletonize_pieces.py; (b) the target of every face component of every
shared plane is a vertex of a tree in both blocks; (c) with fill_holes=False the components are the 26-connected
pieces of the whole volume, one tree per kept piece of tests/pieces_ref.py's flood fill of the whole volume; (d)
child and parent are 26-adjacent and every vertex lies in its label -- (b), (c), (d) on 20 seeded blocky volumes in
a 2 x 2 x 2 grid and on one with a thin last block. Crafted: a thick bar across one cut (one tree, the joint vertex
once, its radius the smaller of the two sides'); the neurite that leaves a block and returns (one tree, no skipped
joint); a ring across a cut (one skipped joint); a blob on the corner of a 2 x 2 grid (one tree); a piece of 2t/3
voxels on each side of a cut is kept and one of t/3 on each side is dropped, which a dust rule per block gets wrong.
A numpy array, an object that only takes three slices and a device tensor give the same arrays; two runs give the
same bits; the output goes through skeleton_to_swc, skeletons_to_zipped_swcs and voxelize_skeletons.
"""

import zipfile

import numpy as np
import pytest
import torch

import blocks_ref
import border_ref
import pieces_ref
from aind_exaspim_neuron_segmentation_amd import inference, segmentation
from test_gpu_dbf import dev  # noqa: F401  (fixture)
from test_gpu_skeletonize_pieces import same_skeletons, volume

pytestmark = pytest.mark.gpu

KW = dict(scale=1.25, const=0.0)


def roots_of(parent):
    """The root row of every row of a forest, by pointer jumping."""
    up = np.where(parent >= 0, parent, np.arange(len(parent)))
    while not np.array_equal(up, up[up]):
        up = up[up]
    return up


def run_with_records(monkeypatch, labels, block_shape, **kw):
    """skeletonize_blocks, the records it hands to join_block_skeletons, and its stats."""
    seen = []
    join = segmentation.join_block_skeletons

    def spy(trees, *args):
        seen.extend(trees)
        return join(trees, *args)

    monkeypatch.setattr(segmentation, "join_block_skeletons", spy)
    stats = {}
    out = inference.skeletonize_blocks(labels, block_shape, stats=stats, **kw)
    monkeypatch.undo()
    return out, seen, stats


def check_d(labels, out):
    for label, (vertices, parent, radius) in out.items():
        assert vertices.dtype == np.int32 and parent.dtype == np.int32 and radius.dtype == np.float32
        assert (labels[tuple(vertices.T)] == label).all()
        inner = parent >= 0
        step = np.abs(vertices[parent[inner]] - vertices[inner]).max(axis=1, initial=0)
        assert (step == 1).all(), label      # 26-adjacent, and never the vertex itself


def check_b(labels, block_shape, records):
    """Every face component of every shared plane has its target as a vertex of a tree in both blocks; the two
    blocks' own views of the plane give the same targets (the seam property)."""
    k = int(labels.max())
    blocks = blocks_ref.grid(labels.shape, block_shape)
    on = {}
    for tree in records:
        voxels = np.ravel_multi_index(tuple(np.asarray(tree["vertices"]).T), labels.shape)
        on.setdefault((tree["block"], tree["label"]), set()).update(voxels.tolist())
    found = 0
    for a, first in enumerate(blocks):
        for face in (1, 3, 5):
            if not first["open"][face]:
                continue
            axis = face // 2
            b = next(i for i, other in enumerate(blocks) if other["lo"][axis] == first["hi"][axis] - 1 and all(
                other["lo"][o] == first["lo"][o] for o in range(3) if o != axis))
            seen = []
            for index, which in ((a, face), (b, face - 1)):
                lo, hi = blocks[index]["lo"], blocks[index]["hi"]
                crop = labels[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
                local = border_ref.face_targets(crop, k, which)
                at = np.array([np.unravel_index(v, crop.shape) for _, v in local], dtype=np.int64).reshape(-1, 3) + lo
                seen.append(sorted(zip([row for row, _ in local],
                                       np.ravel_multi_index(tuple(at.T), labels.shape).tolist())))
            assert seen[0] == seen[1]
            for label, voxel in seen[0]:
                assert voxel in on.get((a, label), ()), (a, label, voxel)
                assert voxel in on.get((b, label), ()), (b, label, voxel)
                found += 1
    return found


def check_c(labels, out, dust):
    """One tree per kept piece of the whole volume, every tree inside its piece."""
    k = int(labels.max())
    pieces, piece_label, _, _, _ = pieces_ref.flood_fill(labels, k, dust)
    assert sorted(out) == sorted(set(piece_label.tolist()))
    for label, (vertices, parent, _) in out.items():
        number = pieces[tuple(vertices.T)]
        root = roots_of(parent)
        assert (number > 0).all() and (number == number[root]).all()      # a tree stays in one piece
        per_tree = number[parent == -1]
        assert sorted(per_tree.tolist()) == (np.flatnonzero(piece_label == label) + 1).tolist()      # each piece once
    return len(piece_label)


# ---- (a) one block ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["y", "comb", "touching", "thick_t", "pieces", "two_ys", "returns"])
def test_one_block_is_skeletonize_pieces(dev, name):      # noqa: F811
    labels = volume(name)
    stats = {}
    got = inference.skeletonize_blocks(labels, (64, 64, 64), dust_threshold=0, stats=stats, **KW)
    want = inference.skeletonize_pieces(labels, dust_threshold=0, **KW)
    same_skeletons(got, want)
    assert list(got) == list(want)
    assert (stats["blocks"], stats["blocks_skipped"], stats["joints"], stats["skipped_joints"]) == (1, 0, 0, 0)
    assert stats["trees"] == sum(int((s[1] == -1).sum()) for s in want.values())
    exact = tuple(max(2, n) for n in labels.shape)
    same_skeletons(inference.skeletonize_blocks(labels, exact, dust_threshold=2, fix_branching=False, fill_holes=False,
                                                **KW),
                   inference.skeletonize_pieces(labels, dust_threshold=2, fix_branching=False, fill_holes=False, **KW))


def test_an_empty_volume_and_the_default_dust(dev):      # noqa: F811
    stats = {}
    assert inference.skeletonize_blocks(np.zeros((5, 6, 7), dtype=np.int32), (4, 4, 4), stats=stats) == {}
    assert (stats["blocks"], stats["blocks_skipped"], stats["trees"]) == (8, 8, 0)
    assert inference.skeletonize_blocks(volume("pieces"), (3, 5, 9)) == {}      # the default is kimimaro's 1000


# ---- crafted cuts -----------------------------------------------------------------------------------------------
def test_a_thick_bar_across_one_cut(dev, monkeypatch):      # noqa: F811
    labels = np.zeros((5, 7, 21), dtype=np.int32)
    labels[1:4, 2:5, 2:11] = 1      # three voxels thick left of the cut and on it ...
    labels[0:5, 1:6, 10:19] = 1      # ... five voxels thick on it and right of it
    out, records, stats = run_with_records(monkeypatch, labels, (5, 7, 11), dust_threshold=0, **KW)
    assert (stats["blocks"], stats["trees"], stats["joints"], stats["skipped_joints"]) == (2, 2, 1, 0)
    vertices, parent, radius = out[1]
    assert list(out) == [1] and (parent == -1).sum() == 1
    assert len(parent) == sum(len(t["parent"]) for t in records) - 1
    joint = np.flatnonzero((vertices == (2, 3, 10)).all(axis=1))
    assert len(joint) == 1      # the centre of the 5 x 5 cut, once
    sides = []
    for tree in records:
        row = np.flatnonzero((np.asarray(tree["vertices"]) == (2, 3, 10)).all(axis=1))
        assert len(row) == 1 and row[0] in tree["border_rows"]
        sides.append(float(tree["radius"][row[0]]))
    assert sides[0] != sides[1] and radius[joint[0]] == np.float32(min(sides))
    assert len(np.unique(vertices, axis=0)) == len(vertices)
    check_d(labels, out)
    assert check_c(labels, out, 0) == 1
    # each side alone is the block's own skeleton: the records are skeletonize_pieces of the crops
    for tree, (x0, x1) in zip(records, ((0, 11), (10, 21))):
        alone = inference.skeletonize_pieces(np.ascontiguousarray(labels[:, :, x0:x1]), dust_threshold=0, **KW)[1]
        np.testing.assert_array_equal(alone[0] + (0, 0, x0), tree["vertices"])
        np.testing.assert_array_equal(alone[1], tree["parent"])
        np.testing.assert_array_equal(alone[2], tree["radius"])


def leaves_and_returns():
    """A neurite that leaves the first block through the cut x = 15 and comes back: a U whose bend lies in the second
    block. The first block sees two pieces of one label, the second one piece that the cut meets twice."""
    labels = np.zeros((5, 16, 30), dtype=np.int32)
    labels[1:4, 2:5, 6:25] = 1
    labels[1:4, 11:14, 3:25] = 1
    labels[1:4, 2:14, 22:25] = 1
    return labels


def test_the_neurite_that_leaves_and_returns(dev, monkeypatch):      # noqa: F811
    labels = leaves_and_returns()
    out, records, stats = run_with_records(monkeypatch, labels, (5, 16, 16), dust_threshold=0, **KW)
    assert (stats["blocks"], stats["trees"], stats["joints"], stats["skipped_joints"]) == (2, 3, 2, 0)
    assert [(t["block"], t["piece"]) for t in records] == [(0, 1), (0, 2), (1, 1)]
    assert (out[1][1] == -1).sum() == 1 and len(out[1][1]) == sum(len(t["parent"]) for t in records) - 2
    check_d(labels, out)
    assert check_b(labels, (5, 16, 16), records) == 2
    assert check_c(labels, out, 0) == 1
    whole = inference.skeletonize_pieces(labels, dust_threshold=0, **KW)
    assert (whole[1][1] == -1).sum() == 1      # the same piece count as the undivided volume; the arrays may differ


def test_a_ring_across_a_cut(dev, monkeypatch):      # noqa: F811
    labels = np.zeros((3, 12, 21), dtype=np.int32)
    labels[1, 2, 3:18] = labels[1, 9, 3:18] = 1
    labels[1, 2:10, 3] = labels[1, 2:10, 17] = 1
    out, records, stats = run_with_records(monkeypatch, labels, (3, 12, 11), dust_threshold=0, **KW)
    assert (stats["blocks"], stats["trees"], stats["joints"], stats["skipped_joints"]) == (2, 2, 2, 1)
    vertices, parent, _ = out[1]
    assert (parent == -1).sum() == 1 and len(parent) == sum(len(t["parent"]) for t in records) - 1
    twice = [v for v in ((1, 2, 10), (1, 9, 10)) if ((vertices == v).all(axis=1)).sum() == 2]
    assert twice == [(1, 9, 10)]      # the joint of larger index is the skipped one
    check_d(labels, out)
    assert check_b(labels, (3, 12, 11), records) == 2
    assert check_c(labels, out, 0) == 1


def test_a_blob_on_the_corner_of_four_blocks(dev, monkeypatch):      # noqa: F811
    labels = np.zeros((4, 13, 13), dtype=np.int32)
    labels[1:3, 4:9, 4:9] = 1
    out, records, stats = run_with_records(monkeypatch, labels, (4, 7, 7), dust_threshold=0, **KW)
    assert (stats["blocks"], stats["trees"]) == (4, 4) and stats["joints"] >= 3
    assert (out[1][1] == -1).sum() == 1
    assert len(out[1][1]) == sum(len(t["parent"]) for t in records) - (stats["trees"] - 1)
    assert sum(t["owned_size"] for t in records) == 50      # every voxel is owned by exactly one block
    check_d(labels, out)
    assert check_b(labels, (4, 7, 7), records) >= 4
    assert check_c(labels, out, 0) == 1


def test_dust_is_judged_across_the_cut(dev, monkeypatch):      # noqa: F811
    """t = 30. A bar of 20 voxels on each side of the cut (39 in all) is kept and one of 10 on each side (19 in all)
    is dropped; bars of 12 and 16 voxels inside a block are dust there already. A dust rule per block drops all
    four."""
    t = 30
    labels = np.zeros((3, 7, 43), dtype=np.int32)
    labels[1, 1, 2:41] = 1
    labels[1, 3, 12:31] = 1
    labels[1, 5, 23:35] = 1
    labels[1, 5, 2:18] = 2
    sizes = pieces_ref.flood_fill(labels, 2)[2]
    assert sorted(sizes.tolist()) == [12, 16, 19, 39]
    out, records, stats = run_with_records(monkeypatch, labels, (3, 7, 22), dust_threshold=t, **KW)
    assert (stats["blocks"], stats["trees"], stats["joints"], stats["skipped_joints"]) == (2, 4, 2, 0)
    assert (stats["open_small_pieces"], stats["dust_components"]) == (4, 1)
    assert [t_["owned_size"] for t_ in records] == [19, 9, 20, 10]      # the plane x = 21 belongs to the second block
    assert list(out) == [1] and (out[1][1] == -1).sum() == 1 and set(out[1][0][:, 1].tolist()) == {1}
    check_d(labels, out)
    assert check_c(labels, out, t) == 1
    for threshold, kept in ((19, 2), (20, 1), (39, 1), (40, 0)):
        got = inference.skeletonize_blocks(labels, (3, 7, 22), dust_threshold=threshold, **KW)
        assert (int((got[1][1] == -1).sum()) if kept else len(got)) == kept
    # what a dust rule per block would give: nothing, although label_pieces of the whole volume keeps one piece
    per_block = [inference.skeletonize_pieces(np.ascontiguousarray(labels[:, :, x0:x1]), dust_threshold=t, **KW)
                 for x0, x1 in ((0, 22), (21, 43))]
    assert per_block == [{}, {}]


# ---- (b), (c), (d) on seeded volumes ----------------------------------------------------------------------------
def blocky(seed):
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(int(v) for v in rng.integers(9, 25, size=3))
    labels = pieces_ref.random_volume(2 * seed + 1, shape, fill=0.3)      # an odd seed: blocks of 2 voxels
    return np.where((labels >= 1) & (labels <= 3), labels, 0).astype(np.int32)


@pytest.mark.parametrize("seed", range(20))
def test_the_properties_on_seeded_volumes(dev, monkeypatch, seed):      # noqa: F811
    labels = blocky(seed)
    block_shape = tuple(n // 2 + 1 for n in labels.shape)
    assert len(blocks_ref.grid(labels.shape, block_shape)) == 8
    dust = 12
    out, records, stats = run_with_records(monkeypatch, labels, block_shape, dust_threshold=dust, fill_holes=False,
                                           **KW)
    assert stats["blocks"] == 8 and stats["trees"] == len(records)
    check_d(labels, out)
    check_b(labels, block_shape, records)
    kept = check_c(labels, out, dust)
    assert kept == sum(int((s[1] == -1).sum()) for s in out.values())
    assert kept + stats["dust_components"] <= stats["trees"]      # the components
    blocks = blocks_ref.grid(labels.shape, block_shape)
    for tree in records:      # the records are what the block alone gives, and own what the reference says
        lo, hi = blocks[tree["block"]]["lo"], blocks[tree["block"]]["hi"]
        crop = labels[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        want = blocks_ref.open_pieces(crop, 3, dust, blocks[tree["block"]]["open"])
        assert tree["label"] == want[1][tree["piece"] - 1]
        assert tree["owned_size"] == blocks_ref.owned_sizes(want[0], len(want[1]), blocks[tree["block"]]["open"])[
            tree["piece"] - 1]


def test_the_seeded_volumes_hold_what_they_are_for():
    """Without a GPU: cuts through pieces, pieces in several blocks, small open pieces and dust of both kinds."""
    cut = small = whole_dust = 0
    for seed in range(20):
        labels = blocky(seed)
        block_shape = tuple(n // 2 + 1 for n in labels.shape)
        pieces = pieces_ref.flood_fill(labels, 3)
        whole_dust += int((pieces[2] < 12).sum())
        for block in blocks_ref.grid(labels.shape, block_shape):
            lo, hi = block["lo"], block["hi"]
            want = blocks_ref.open_pieces(labels[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], 3, 12, block["open"])
            cut += int(want[4].sum())
            small += want[6]
    assert cut >= 100 and small >= 40 and whole_dust >= 20, (cut, small, whole_dust)


def test_a_thin_last_block(dev, monkeypatch):      # noqa: F811
    labels = pieces_ref.random_volume(77, (7, 9, 16), fill=0.4)
    labels = np.where((labels >= 1) & (labels <= 3), labels, 0).astype(np.int32)
    block_shape = (7, 9, 8)
    assert blocks_ref.spans(16, 8) == [(0, 8), (7, 15), (14, 16)]
    out, records, stats = run_with_records(monkeypatch, labels, block_shape, dust_threshold=6, fill_holes=False, **KW)
    assert stats["blocks"] == 3 and {t["block"] for t in records} == {0, 1, 2}
    check_d(labels, out)
    assert check_b(labels, block_shape, records) >= 1
    assert check_c(labels, out, 6) >= 1


# ---- inputs, determinism, output --------------------------------------------------------------------------------
class SlicesOnly:
    """What a zarr array or a memmap offers at the least: shape, dtype and three-slice indexing."""

    def __init__(self, array):
        self._array, self.shape, self.dtype, self.reads = array, array.shape, array.dtype, []

    def __getitem__(self, key):
        assert isinstance(key, tuple) and len(key) == 3, key
        assert all(isinstance(s, slice) and s.step is None and 0 <= s.start < s.stop for s in key), key
        self.reads.append(tuple((s.start, s.stop) for s in key))
        return self._array[key]


def test_the_three_kinds_of_input_and_two_runs(dev):      # noqa: F811
    labels = leaves_and_returns()
    kw = dict(dust_threshold=0, **KW)
    base = inference.skeletonize_blocks(labels, (5, 9, 16), **kw)
    source = SlicesOnly(labels)
    from_slices = inference.skeletonize_blocks(source, (5, 9, 16), **kw)
    assert source.reads == [tuple(zip(b["lo"], b["hi"])) for b in blocks_ref.grid(labels.shape, (5, 9, 16))]
    on_device = inference.skeletonize_blocks(torch.from_numpy(labels).to(dev), (5, 9, 16), device=dev, **kw)
    again = inference.skeletonize_blocks(labels, (5, 9, 16), device="cuda:0", **kw)
    for other in (from_slices, on_device, again):
        assert list(other) == list(base) == [1]
        for a, b in zip(other[1], base[1]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.skeletonize_blocks(torch.from_numpy(labels), (5, 9, 16))
    with pytest.raises(TypeError, match="int32"):
        inference.skeletonize_blocks(torch.from_numpy(labels).to(dev).to(torch.int64), (5, 9, 16))


def test_the_output_goes_through_the_writers(dev, tmp_path):      # noqa: F811
    labels = leaves_and_returns()
    labels[2, 7:9, 0:30] = 2
    stats = {}
    got = inference.skeletonize_blocks(labels, (5, 16, 16), dust_threshold=0, stats=stats, **KW)
    for key in ("blocks", "blocks_skipped", "trees", "joints", "skipped_joints", "dust_components",
                "open_small_pieces", "chain_seconds", "join_seconds"):
        assert key in stats, key
    assert stats["chain_seconds"] > 0 and stats["join_seconds"] > 0 and sorted(got) == [1, 2]
    text = inference.skeleton_to_swc(*got[1])
    lines = [line.split() for line in text.splitlines()]
    assert len(lines) == len(got[1][1]) and sum(line[6] == "-1" for line in lines) == 1
    path = tmp_path / "blocks.zip"
    inference.skeletons_to_zipped_swcs(got, path)
    with zipfile.ZipFile(path) as archive:
        assert sorted(archive.namelist()) == ["1.swc", "2.swc"]
        assert archive.read("1.swc").decode() == text
    img = inference.voxelize_skeletons(got, labels.shape)
    np.testing.assert_array_equal(img[img > 0], labels[img > 0])
    voxels = np.concatenate([np.ravel_multi_index(tuple(s[0].T), labels.shape) for s in got.values()])
    assert (img > 0).sum() == len(np.unique(voxels))      # both sides of a cut may walk the shared plane
