"""
inference.skeletonize_pieces on the GPU (-m gpu), on the small volumes of tests/fix_borders_ref.py (the Y, the comb,
touching labels, a label in pieces with one-voxel labels, the thick T) at that file's small scale and const:
(i) where tests/pieces_ref.py confirms that every label is one piece, it is skeletonize_fix_borders, and with
fix_borders=False skeletonize, array for array; (ii) with several pieces per label it is composed from existing
parts: device fill_holes, the oracle's pieces on the host, skeletonize_fix_borders of the piece volume, regrouped
on the host; (iii) every border target in a kept piece is a vertex of its label's forest, and skeletonize_fix_borders
misses at least one on the same volume; (iv) a label that is only dust is absent and dust next to a kept piece
changes none of its arrays; (v) max_paths counts per piece; (vi) forests go through skeleton_to_swc,
skeletons_to_zipped_swcs and voxelize_skeletons; (vii) the older functions give what they gave; (viii) two runs
give the same bits.
"""

import zipfile

import numpy as np
import pytest

import border_ref
import fix_borders_ref as fx
import pieces_ref
from aind_exaspim_neuron_segmentation_amd import inference
from test_gpu_dbf import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

KW = dict(scale=1.25, const=0.0)
_VOLUMES = {}


def two_ys():
    """The Y of fix_borders_ref twice under one label, four planes apart, and a bar of label 2 between them: label 1
    is two pieces with three ends on faces each, the second mirrored so that the trees differ."""
    y = np.array(fx.faces_y()[0])[0]
    labels = np.zeros((5,) + y.shape, dtype=np.int32)
    labels[0] = y
    labels[4] = y[::-1]
    labels[2, 3, :] = 2
    return labels


def leaves_and_returns():
    """A neurite that leaves the block through the face x = W - 1 and comes back: two bars of label 1, three voxels
    thick, that both start on x = W - 1; the upper one turns and ends on y = 0. Label 2 lies between them."""
    labels = np.zeros((5, 16, 20), dtype=np.int32)
    labels[1:4, 2:5, 6:20] = 1
    labels[1:4, 0:2, 6:9] = 1
    labels[1:4, 11:14, 3:20] = 1
    labels[2, 7:9, 0:20] = 2
    return labels


def volume(name):
    """A writable copy of the shared volume, which is made once and left unchanged."""
    if name not in _VOLUMES:
        made = {"two_ys": two_ys, "returns": leaves_and_returns}
        labels = made[name]() if name in made else np.array(fx.CASES[name]()[0])
        labels.setflags(write=False)
        _VOLUMES[name] = labels
    return _VOLUMES[name].copy()


def same_skeletons(got, want):
    assert sorted(got) == sorted(want)
    for row in want:
        assert len(got[row]) == len(want[row]) == 3
        for a, b in zip(got[row], want[row]):
            assert a.dtype == b.dtype and a.shape == b.shape, row
            np.testing.assert_array_equal(a, b, err_msg=f"label {row}")


def composed(labels, dust, **kw):
    """The expected forests from existing parts: fill_holes on the device, the oracle's pieces on the host,
    skeletonize_fix_borders of the piece volume, and the regrouping rule written out."""
    filled = inference.fill_holes(np.array(labels))
    pieces, piece_label, _, _, _ = pieces_ref.flood_fill(filled, max(int(filled.max()), 0), dust)
    if len(piece_label) == 0:
        return {}, pieces, piece_label
    trees = inference.skeletonize_fix_borders(pieces, fill_holes=False, **kw)
    out = {}
    for label in sorted(set(piece_label.tolist())):
        vertices, parent, radius, rows = [], [], [], 0
        for number in np.flatnonzero(piece_label == label) + 1:      # ascending piece number
            if int(number) not in trees:
                continue
            v, p, r = trees[int(number)]
            assert (p == -1).sum() == 1
            vertices.append(v)
            parent.append(np.where(p >= 0, p + rows, -1).astype(np.int32))
            radius.append(r)
            rows += len(p)
        if vertices:
            out[label] = (np.concatenate(vertices), np.concatenate(parent), np.concatenate(radius))
    return out, pieces, piece_label


# ---- (i) connected labels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["y", "comb", "touching", "thick_t"])
def test_connected_labels_get_the_skeletons_of_skeletonize_fix_borders(dev, name):      # noqa: F811
    labels = volume(name)
    k = int(labels.max())
    assert pieces_ref.flood_fill(labels, k)[1].tolist() == list(range(1, k + 1))      # every label is one piece
    for kw in (KW, dict(scale=0.0, const=2.0)):
        same_skeletons(inference.skeletonize_pieces(labels, dust_threshold=0, **kw),
                       inference.skeletonize_fix_borders(labels, **kw))
        same_skeletons(inference.skeletonize_pieces(labels, dust_threshold=0, fix_borders=False, **kw),
                       inference.skeletonize(labels, **kw))
    same_skeletons(inference.skeletonize_pieces(labels, dust_threshold=0, fix_branching=False, **KW),
                   inference.skeletonize_fix_borders(labels, fix_branching=False, **KW))


# ---- (ii) several pieces per label ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pieces", "two_ys", "returns"])
@pytest.mark.parametrize("fix_branching", [True, False])
def test_several_pieces_per_label_against_the_composition(dev, name, fix_branching):      # noqa: F811
    labels = volume(name)
    want, pieces, piece_label = composed(labels, 0, fix_branching=fix_branching, **KW)
    assert len(piece_label) > len(set(piece_label.tolist()))      # a label in more than one piece
    got = inference.skeletonize_pieces(labels, dust_threshold=0, fix_branching=fix_branching, **KW)
    same_skeletons(got, want)
    assert (got[1][1] == -1).sum() == (piece_label == 1).sum() == 2      # a forest of two trees
    for row, (vertices, parent, radius) in got.items():      # every tree stays inside its piece
        number = pieces[tuple(vertices.T)]
        assert (piece_label[number - 1] == row).all()
        inner = parent >= 0
        assert (number[parent[inner]] == number[inner]).all() and (np.diff(number) >= 0).all()


# ---- (iii) border targets: the feature --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pieces", "two_ys", "returns"])
def test_every_border_target_in_a_kept_piece_is_a_vertex(dev, name):      # noqa: F811
    labels = volume(name)
    k = int(labels.max())
    filled = inference.fill_holes(np.array(labels))
    rows = border_ref.by_component(filled, k)
    assert len(rows) >= 3

    def missed(skeletons):
        out = []
        for label, voxel in rows.tolist():
            on = set() if label not in skeletons else set(
                np.ravel_multi_index(tuple(skeletons[label][0].T), labels.shape).tolist())
            if voxel not in on:
                out.append((label, voxel))
        return out

    assert missed(inference.skeletonize_pieces(labels, dust_threshold=0, **KW)) == []
    old = missed(inference.skeletonize_fix_borders(labels, **KW))
    assert len(old) >= 1 and all(label == 1 for label, _ in old)      # the pieces the root does not reach


# ---- (iv) dust --------------------------------------------------------------------------------------------------
def test_dust(dev):      # noqa: F811
    labels = volume("pieces")      # labels 2 and 3 are one voxel each, label 4 is 12 voxels, label 1 is 2 x 36
    got = inference.skeletonize_pieces(labels, dust_threshold=2, **KW)
    assert sorted(got) == [1, 4]
    same_skeletons(got, composed(labels, 2, **KW)[0])
    assert sorted(inference.skeletonize_pieces(labels, dust_threshold=13, **KW)) == [1]
    assert inference.skeletonize_pieces(labels, dust_threshold=37, **KW) == {}
    assert inference.skeletonize_pieces(np.zeros((3, 4, 5), dtype=np.int32)) == {}
    assert inference.skeletonize_pieces(labels) == {}      # the default is kimimaro's 1000
    # dust next to a kept piece: two voxels of label 1 one voxel away from the T, one voxel of label 2 touching it
    clean = np.array(volume("thick_t"))
    dusty = clean.copy()
    assert not dusty[1:4, 8:11, 24:26].any() and dusty[2, 8, 22] == 1 and not dusty[0, 4, 10] and dusty[1, 4, 10] == 1
    dusty[2, 9, 24:26] = 1
    dusty[0, 4, 10] = 2
    assert sorted(pieces_ref.flood_fill(dusty, 2)[2].tolist())[:2] == [1, 2]
    assert pieces_ref.flood_fill(dusty, 2, 5)[4] == 2
    for fix_borders in (True, False):
        want = inference.skeletonize_pieces(clean, dust_threshold=5, fix_borders=fix_borders, **KW)
        got = inference.skeletonize_pieces(dusty, dust_threshold=5, fix_borders=fix_borders, **KW)
        assert sorted(got) == [1]
        same_skeletons(got, want)
    assert sorted(inference.skeletonize_pieces(dusty, dust_threshold=0, **KW)) == [1, 2]


# ---- (v) max_paths ----------------------------------------------------------------------------------------------
def test_max_paths_counts_per_piece(dev):      # noqa: F811
    labels = volume("two_ys")
    full = inference.skeletonize_pieces(labels, dust_threshold=0, **KW)
    for max_paths in (1, 2):
        got = inference.skeletonize_pieces(labels, dust_threshold=0, max_paths=max_paths, **KW)
        same_skeletons(got, composed(labels, 0, max_paths=max_paths, **KW)[0])
        vertices, parent, _ = got[1]
        assert (parent == -1).sum() == 2 and len(parent) <= len(full[1][1])
        if max_paths == 1:
            assert len(parent) < len(full[1][1])      # a Y is more than one path
        planes = vertices[:, 0]
        assert set(planes.tolist()) == {0, 4}      # both pieces got their paths, not the first alone
        # a tree of max_paths paths has at most max_paths leaves besides its root
        leaves = np.setdiff1d(np.arange(len(parent)), parent[parent >= 0])
        assert len(leaves) <= 2 * max_paths + 2


# ---- (vi) the output functions ----------------------------------------------------------------------------------
def test_forests_go_through_the_output_functions(dev, tmp_path):      # noqa: F811
    labels = volume("two_ys")
    got = inference.skeletonize_pieces(labels, dust_threshold=0, **KW)
    vertices, parent, radius = got[1]
    text = inference.skeleton_to_swc(vertices, parent, radius)
    lines = [line.split() for line in text.splitlines()]
    assert len(lines) == len(parent) and [int(line[0]) for line in lines] == list(range(1, len(parent) + 1))
    assert [int(line[6]) for line in lines] == [p + 1 if p >= 0 else -1 for p in parent.tolist()]
    assert sum(line[6] == "-1" for line in lines) == 2
    path = tmp_path / "forests.zip"
    inference.skeletons_to_zipped_swcs(got, path)
    with zipfile.ZipFile(path) as archive:
        assert sorted(archive.namelist()) == ["1.swc", "2.swc"]
        assert archive.read("1.swc").decode() == text
    img = inference.voxelize_skeletons(got, labels.shape)
    assert img.shape == labels.shape and set(np.unique(img).tolist()) == {0, 1, 2}
    np.testing.assert_array_equal(img[img > 0], labels[img > 0])
    assert (img[0] == 1).any() and (img[4] == 1).any() and (img > 0).sum() == sum(len(s[1]) for s in got.values())


# ---- (vii) the older functions ----------------------------------------------------------------------------------
def test_the_older_functions_are_unchanged(dev):      # noqa: F811
    labels = volume("two_ys")
    before = (inference.skeletonize(labels, **KW), inference.skeletonize_labels(labels, **KW),
              inference.skeletonize_fix_borders(labels, **KW))
    inference.skeletonize_pieces(labels, dust_threshold=0, **KW)
    after = (inference.skeletonize(labels, **KW), inference.skeletonize_labels(labels, **KW),
             inference.skeletonize_fix_borders(labels, **KW))
    for a, b in zip(before, after):
        same_skeletons(a, b)
    for skeletons in after:      # one root per label: the root's piece alone, as their docstrings say
        assert sorted(skeletons) == [1, 2] and (skeletons[1][1] == -1).sum() == 1
        assert len(set(skeletons[1][0][:, 0].tolist())) == 1
    same_skeletons(inference.skeletonize_fix_borders(labels, fix_borders=False, **KW), after[0])
    # the root's piece gets the same tree in both forms: the first tree of the forest or the second
    forest = inference.skeletonize_pieces(labels, dust_threshold=0, **KW)[1]
    old = after[2][1]
    plane = int(old[0][0, 0])
    mine = forest[0][:, 0] == plane
    np.testing.assert_array_equal(forest[0][mine], old[0])
    np.testing.assert_array_equal(forest[2][mine], old[2])


# ---- (viii) determinism -----------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(dev):      # noqa: F811
    labels = volume("returns")
    a = inference.skeletonize_pieces(labels, dust_threshold=0, **KW)
    b = inference.skeletonize_pieces(labels, dust_threshold=0, **KW)
    assert sorted(a) == sorted(b) == [1, 2]
    for row in a:
        assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a[row], b[row]))
