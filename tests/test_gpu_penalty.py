"""
Stage 6 of skeletonize_labels on the GPU (-m gpu): the penalty field that torch float32 arithmetic builds on
the device, against the float64 oracle of tests/penalty_ref.py fed with the chain's own dbf and daf (both
bit-checked against their oracles here), within penalty_ref.bound, on six volumes and four parameter cases that
isolate the terms. Then the whole chain on the volumes test_gpu_teasar.py does not run -- absent ids, one-voxel
labels and a thin line across tile seams, labels in pieces, one label filling the volume, a single plane --
against the composed oracles, skeletonize_labels against properties that need no oracle of the project's, and
the reference's default const=450, at which every label has one path.

Measured on an MI355X, worst |cost - ref| / bound over the volumes: pdrf_scale=0 0.016 (bit-equal to numpy's float32
quotient), pdrf_exponent=0 0.041, pdrf_exponent=1 0.055, the defaults 0.038. The test prints each.
"""

import numpy as np
import pytest
import torch

import geodesic_ref as ref
import holes_ref
import parents_ref as pref
import penalty_ref as pen
import teasar_ref as tref
from test_gpu_teasar import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# (pdrf_exponent, pdrf_scale): one float32 division alone; scale + daf / far; a plain product; the defaults
CASES = {"scale0": (4, 0.0), "exponent0": (0, 100000.0), "exponent1": (1, 100000.0), "defaults": (4, 100000.0)}
SCALE, CONST = 1.25, 2.0      # the invalidation of test_skeletonize_labels_against_the_oracles
NAMES = sorted(pen.VOLUMES)


@pytest.fixture(scope="module")
def front(dev):  # noqa: F811
    """Per volume, computed once and only read: the oracles of the stages before the penalty."""
    cache = {}

    def get(name):
        if name not in cache:
            labels = pen.VOLUMES[name]()
            filled, _ = holes_ref.by_components(labels)
            filled = np.ascontiguousarray(filled, dtype=np.int32)
            k = max(int(filled.max()), 0)
            dbf = tref.dbf_of(filled)
            first = ref.first_voxels(filled, k)
            _, roots = ref.farthest(filled, first, ref.relaxation(filled, first))
            daf = ref.relaxation(filled, roots)
            far_value, far_index = ref.farthest(filled, roots, daf)
            entry = dict(labels=labels, filled=filled, k=k, dbf=dbf, roots=roots, daf=daf, far_index=far_index)
            for a in entry.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cache[name] = entry
        return cache[name]

    yield get
    cache.clear()


def run_chain(dev, labels, exponent, scale, const=CONST, max_paths=None):  # noqa: F811
    from aind_exaspim_neuron_segmentation_amd import inference

    return inference._skeleton_chain_on_device(torch.from_numpy(np.array(labels)).to(dev), SCALE, const, exponent, scale,
                                               True, max_paths)


def check_front(chain, want):
    """The chain's inputs of the penalty are their oracles', bit for bit."""
    np.testing.assert_array_equal(chain["labels"].cpu().numpy(), want["filled"])
    np.testing.assert_array_equal(chain["dbf"].cpu().numpy(), want["dbf"])
    np.testing.assert_array_equal(chain["roots"].cpu().numpy(), want["roots"])
    np.testing.assert_array_equal(ref.bits(chain["daf"].cpu().numpy()), ref.bits(want["daf"]))


# ---- 1. the penalty --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_penalty_field_against_the_float64_oracle(dev, front, name):  # noqa: F811
    want = front(name)
    filled, k = want["filled"], want["k"]
    assert filled.size <= 30000
    inside = pen.inside_of(filled, k)
    at_defaults = None
    for case, (exponent, scale) in CASES.items():
        chain = run_chain(dev, want["labels"], exponent, scale, max_paths=1)
        check_front(chain, want)
        dbf, daf = chain["dbf"].cpu().numpy(), chain["daf"].cpu().numpy()
        cost = chain["cost"].cpu().numpy()
        assert cost.dtype == np.float32 and cost.shape == filled.shape
        oracle = pen.cost(filled, dbf, daf, k, exponent, scale)
        ratio = pen.worst_ratio(cost, oracle, filled, k, exponent, scale)      # NaN and +inf are checked inside
        note = ""
        peak, far = pen.maxima(filled, dbf, daf, k)
        rows = np.where(inside, filled, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            quotient = np.where(far[rows] > 0, daf / far[rows].astype(np.float32), np.float32(0)).astype(np.float32)
        if case == "scale0":
            # one float32 division: within 1 ulp of numpy's float32 quotient
            finite = inside & np.isfinite(quotient)
            ulps = np.abs(ref.bits(cost)[finite].astype(np.int64) - ref.bits(quotient)[finite].astype(np.int64))
            note = f", ulps off the float32 quotient: {int(ulps.max(initial=0))} (bit-equal: {not ulps.any()})"
            assert ulps.max(initial=0) <= 1
            assert (cost[inside & np.isinf(quotient)] == np.inf).all()
        if case == "exponent0":
            some = inside & (peak[rows] > 0) & np.isfinite(oracle)
            assert some.any()
            divisor = far[rows][some]
            second = np.where(divisor > 0, daf[some].astype(np.float64) / np.where(divisor > 0, divisor, 1.0), 0.0)
            np.testing.assert_array_equal(oracle[some], scale + second)      # the oracle: pdrf_scale + daf / far
            assert np.abs(cost[some] - (scale + second)).max() <= pen.bound(0, scale)
        print(f"penalty, volume {name}, {case} (e={exponent}, scale={scale:g}): worst |cost - ref| / bound = "
              f"{ratio:.4f}{note}")
        assert ratio <= 1.0, (name, case, ratio)
        if case == "defaults":
            at_defaults = dict(cost=cost, far=far, oracle=oracle, dbf=dbf)
    cost, far, oracle, dbf = (at_defaults[key] for key in ("cost", "far", "oracle", "dbf"))      # what follows: (4, 1e5)
    if name == "b":
        assert sorted(np.unique(filled[filled > 0]).tolist()) == [1, 3, 6] and k == 6
    if name == "c":
        assert (far[[1, 3, 4]] == 0).all() and far[2] == 69.0 and (cost[filled == 1] == 0).all()
    if name == "d":
        assert np.isinf(oracle[filled == 1]).any() and np.isfinite(oracle[filled == 1]).any()
        assert np.isfinite(oracle[filled == 2]).all()
    if name == "e":
        assert (dbf == tref.DBF_INF).all() and (cost <= 1.0).all() and (cost >= 0).all()      # defaults: no first term


# ---- 2. the chain on those volumes -----------------------------------------------------------------------------
def composed(dev, front, name):  # noqa: F811
    """One run of the chain at the defaults of the penalty and (SCALE, CONST), held to the composed oracles as
    test_skeletonize_labels_against_the_oracles holds it."""
    want = front(name)
    filled, k = want["filled"], want["k"]
    chain = run_chain(dev, want["labels"], 4, 100000.0)
    check_front(chain, want)
    cost = chain["cost"].cpu().numpy()      # held to its oracle above; an input of what follows
    field = ref.relaxation(filled, want["roots"], cost)
    parents, hops, orphans, invalid = pref.jacobi(filled, want["roots"], field, cost)
    assert invalid == 0
    np.testing.assert_array_equal(chain["parents"].cpu().numpy(), parents)
    np.testing.assert_array_equal(chain["hops"].cpu().numpy(), hops)
    np.testing.assert_array_equal(chain["boxes"].cpu().numpy(), tref.boxes_of(filled, k))
    result = tref.incremental(filled, want["roots"], want["dbf"], want["daf"], parents, hops, SCALE, CONST)
    for key, b in zip(("voxels", "radii", "offsets", "branch_label", "branch_round", "branch_junction"),
                      result.arrays()):
        np.testing.assert_array_equal(chain[key].cpu().numpy(), b, err_msg=key)
    assert chain["before"].cpu().tolist() == result.before
    return dict(result=result, parents=parents, hops=hops)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "a"])      # (a) is test_gpu_teasar.py's
def test_the_chain_against_the_composed_oracles(dev, front, name):  # noqa: F811
    want, got = front(name), composed(dev, front, name)
    result, k = got["result"], want["k"]
    present = [row for row in range(1, k + 1) if (want["filled"] == row).any()]
    assert sorted(set(result.branch_label)) == present      # every label has a root, so every label has a skeleton
    if name == "c":
        line = result.branch_label.index(2)
        assert result.offsets[line + 1] - result.offsets[line] == 70      # the whole line, across both seams
    if name == "d":
        away = (want["filled"] == 1) & ~np.isfinite(want["daf"])      # the piece of label 1 its root does not reach
        assert away.any() and (got["hops"][away] == -1).all() and (got["parents"][away] == -1).all()
    if name == "e":
        assert len(result.states) == 1 and set(result.radii) == {40}


@pytest.mark.parametrize("const", [CONST, 0.0])      # 0.0: many rounds, radii down to 1
@pytest.mark.parametrize("name", NAMES)
def test_skeletons_have_the_properties_that_need_no_oracle(dev, front, name, const):  # noqa: F811
    from aind_exaspim_neuron_segmentation_amd import inference

    want = front(name)
    filled, dbf, shape = want["filled"], want["dbf"], want["filled"].shape
    cap = max(shape)
    skeletons = inference.skeletonize_labels(np.array(want["labels"]), scale=SCALE, const=const)
    assert sorted(skeletons) == sorted(np.unique(filled[filled > 0]).tolist())
    grid = np.indices(shape)
    for row, (vertices, parent, radius) in skeletons.items():
        n = len(vertices)
        at = tuple(vertices.T)
        assert (filled[at] == row).all()                                            # every vertex lies in its label
        assert parent[0] == -1 and (parent[1:] >= 0).all() and (parent[1:] < n).all()      # row 0 is the only root
        assert np.ravel_multi_index(at, shape)[0] == want["roots"][row]
        assert len({tuple(v) for v in vertices.tolist()}) == n
        step = np.abs(vertices[1:] - vertices[parent[1:]]).max(axis=1, initial=0)
        assert (step == 1).all()                                                    # 26-adjacent to the parent
        up, steps = np.arange(n), 0
        while (up != 0).any():                                                      # parents lead to row 0
            up = np.where(up != 0, parent[up], 0)
            steps += 1
            assert steps < n, "a cycle"
        np.testing.assert_array_equal(radius, np.sqrt(dbf[at].astype(np.float32)))
        assert np.isfinite(radius).all()
        # nothing was invalidated for free: every voxel of the root's piece is inside some vertex's cube
        reach = tref.radius(dbf[at], SCALE, const, cap)
        piece = (filled == row) & np.isfinite(want["daf"])
        covered = np.zeros(shape, dtype=bool)
        for v, r in zip(vertices, reach):
            covered |= np.abs(grid - v.reshape(3, 1, 1, 1)).max(axis=0) <= r
        assert not (piece & ~covered).any()
        if name == "d" and row == 1:
            away = (filled == 1) & ~np.isfinite(want["daf"])
            assert away.any() and not away[at].any()      # the piece the root does not touch has no vertex
    if name == "e":
        assert all(np.isfinite(r).all() and not np.isnan(r).any() for _, _, r in skeletons.values())
    # nothing was left valid that should not be: no path's target lies in the cube of a vertex of an earlier round
    chain = run_chain(dev, want["labels"], 4, 100000.0, const=const)
    voxels, radii, offsets, branch_label, branch_round = (
        chain[key].cpu().numpy() for key in ("voxels", "radii", "offsets", "branch_label", "branch_round"))
    assert len(voxels) == sum(len(v[0]) for v in skeletons.values())
    rows, rounds = np.repeat(branch_label, np.diff(offsets)), np.repeat(branch_round, np.diff(offsets))
    coords = np.stack(np.unravel_index(voxels.astype(np.int64), shape), axis=1)
    np.testing.assert_array_equal(radii, tref.radius(dbf.reshape(-1)[voxels], SCALE, const, cap))
    later = 0
    for b in range(len(branch_label)):
        target = coords[offsets[b + 1] - 1]
        earlier = (rows == branch_label[b]) & (rounds < branch_round[b])
        if earlier.any():
            later += 1
            apart = np.abs(coords[earlier] - target).max(axis=1)
            assert (apart > radii[earlier]).all(), (name, b)
    if name in "abf" and const == 0.0:
        assert later >= 2      # the property is live
    elif name in "af":
        assert later >= 1


@pytest.mark.parametrize("name", NAMES)
def test_the_references_defaults_give_one_path_per_label(dev, front, name):  # noqa: F811
    """const=450 is larger than any volume here: one round, a path from the root to ref.farthest's voxel."""
    from aind_exaspim_neuron_segmentation_amd import inference

    want = front(name)
    filled, shape = want["filled"], want["filled"].shape
    chain = inference._skeleton_chain_on_device(torch.from_numpy(np.array(want["labels"])).to(dev), 1.25, 450.0, 4,
                                                100000.0, True, None)
    labels_of = chain["branch_label"].cpu().tolist()
    offsets, voxels = chain["offsets"].cpu().tolist(), chain["voxels"].cpu().tolist()
    present = sorted(np.unique(filled[filled > 0]).tolist())
    assert labels_of == present and set(chain["branch_round"].cpu().tolist()) <= {1}
    assert set(chain["branch_junction"].cpu().tolist()) <= {-1}
    for b, row in enumerate(labels_of):
        assert voxels[offsets[b]] == want["roots"][row] and voxels[offsets[b + 1] - 1] == want["far_index"][row]
    skeletons = inference.skeletonize_labels(np.array(want["labels"]))      # every default
    assert sorted(skeletons) == present
    for b, row in enumerate(labels_of):
        vertices, parent, _ = skeletons[row]
        index = np.ravel_multi_index(tuple(vertices.T), shape)
        assert index[0] == want["roots"][row] and want["far_index"][row] in index.tolist()
        assert len(index) == offsets[b + 1] - offsets[b] and np.bincount(parent[1:], minlength=len(index)).max(initial=0) <= 1
    stats = {}
    from aind_exaspim_neuron_segmentation_amd import segmentation

    out = segmentation.teasar_branches(chain["labels"], chain["roots"], chain["dbf"], chain["daf"], chain["parents"],
                                       chain["hops"], scale=1.25, const=450.0, stats=stats)
    assert stats["rounds"] == 1 and out[0].tolist() == voxels
