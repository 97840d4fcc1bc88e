"""
Given targets in TEASAR's loops on the GPU (-m gpu): exaspim_teasar_round_given through the C ABI next to
exaspim_teasar_round (every row -1: the same bytes; a target on the skeleton: no branch, not finished; refused rows:
counted and read as -1), and inference.teasar_branches_given, teasar_branches_fix_branching_given and
skeletonize_fix_borders against tests/fix_borders_ref.py: the state volume after every round in both forms on the
Y, the comb, touching labels, a label in pieces with one-voxel labels and the thick T, all cut by faces, with
inference.border_targets' result as the given targets; None is today's call; the chain against the composed
oracles; skeletonize unchanged; max_paths inside the given rounds; determinism. Nothing here provokes a fault:
every given row the kernel refuses is range-checked before it is used as an index.
"""

import numpy as np
import pytest
import torch

import border_ref
import fix_borders_ref as fx
import geodesic_ref as ref
import holes_ref
import penalty_ref
import teasar_ref as tref
from aind_exaspim_neuron_segmentation_amd import _native, inference
from test_gpu_dbf import dev, guarded, intact  # noqa: F401  (fixture and helpers)

pytestmark = pytest.mark.gpu

_CASES = {}


def case(name):
    """The shared case, left unchanged: (labels, sources, dbf, daf, cost)."""
    if name not in _CASES:
        inputs = fx.CASES[name]()
        for a in inputs:
            a.setflags(write=False)
        _CASES[name] = inputs
    return _CASES[name]


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------
class Rounds:
    """exaspim_teasar_begin on a case's device fields, and the two round entries into guarded 0xFF buffers."""

    def __init__(self, dev, inputs):      # noqa: F811
        self.dev, self.lib = dev, _native.lib()
        labels, sources, dbf, daf, cost = (torch.from_numpy(np.array(a)).to(dev) for a in inputs)
        field, _, _ = inference._geodesic_on_device(labels, sources, cost)
        self.parents, self.hops = inference._geodesic_parents_on_device(labels, sources, field, cost)
        self.labels, self.sources, self.dbf, self.daf = labels, sources, dbf, daf
        self.k = int(sources.numel()) - 1
        self.dims = _native.int3(tuple(labels.shape))
        self.boxes = inference.segment_table(labels, n_labels=self.k, return_device_tensors=True)[1]
        self.need = self.lib.exaspim_teasar_workspace_bytes(self.dims, self.k)
        self.workspace = torch.zeros(self.need, dtype=torch.uint8, device=dev)
        self.mask = torch.zeros(tuple(labels.shape), dtype=torch.uint8, device=dev)
        self.state = torch.zeros(6, dtype=torch.int32, device=dev)
        rc = self.lib.exaspim_teasar_begin(labels.data_ptr(), sources.data_ptr(), self.hops.data_ptr(), daf.data_ptr(),
                                           self.dims, self.k, self.mask.data_ptr(), self.state.data_ptr(),
                                           self.workspace.data_ptr(), self.need, None)
        assert rc == 0, _native.last_error()

    def round(self, given=None):
        """One call on copies of the state words and the workspace: (targets, lengths, junction, state words)."""
        rows = self.k + 1
        full_t, targets = guarded(self.dev, rows, torch.int32)
        full_l, lengths = guarded(self.dev, rows, torch.int64)
        full_j, junction = guarded(self.dev, rows, torch.int32)
        full_s, state = guarded(self.dev, 6, torch.int32)
        state[:5] = self.state[:5]      # the sixth word stays 0xFF for the old entry, which must not touch it
        workspace = self.workspace.clone()
        head = (self.labels.data_ptr(), self.daf.data_ptr(), self.parents.data_ptr(), self.hops.data_ptr(), self.dims,
                self.k, self.mask.data_ptr())
        tail = (targets.data_ptr(), lengths.data_ptr(), junction.data_ptr(), state.data_ptr(), workspace.data_ptr(),
                self.need, None)
        if given is None:
            rc = self.lib.exaspim_teasar_round(*head, *tail)
        else:
            row = torch.tensor(given, dtype=torch.int32, device=self.dev)
            assert row.numel() == rows
            rc = self.lib.exaspim_teasar_round_given(*head, row.data_ptr(), *tail)
        torch.cuda.synchronize()
        assert rc == 0, _native.last_error()
        assert intact(full_t, rows, torch.int32) and intact(full_l, rows, torch.int64)
        assert intact(full_j, rows, torch.int32) and intact(full_s, 6, torch.int32)
        self.last = (targets, lengths, junction, state, workspace)
        return tuple(t.cpu().numpy() for t in (targets, lengths, junction, state))

    def apply(self):
        """exaspim_teasar_apply of the last round() call, whose state words and workspace become the loop's."""
        targets, lengths, junction, state, workspace = self.last
        self.state[:5] = state[:5]
        self.workspace = workspace
        live, broken, n_new, n_roots = (int(v) for v in state[:4].cpu())
        assert broken == 0
        offsets = torch.zeros(self.k + 2, dtype=torch.int64, device=self.dev)
        torch.cumsum(lengths, 0, out=offsets[1:])
        voxels, radii, before = (torch.zeros(max(n_new, 1), dtype=torch.int32, device=self.dev) for _ in range(3))
        rc = self.lib.exaspim_teasar_apply(self.labels.data_ptr(), self.parents.data_ptr(), self.dbf.data_ptr(),
                                           self.boxes.data_ptr(), self.dims, self.k, 1.25, 0.0, self.mask.data_ptr(),
                                           targets.data_ptr(), lengths.data_ptr(), junction.data_ptr(),
                                           offsets.data_ptr(), voxels.data_ptr(), radii.data_ptr(), before.data_ptr(),
                                           n_new, n_new, n_roots, self.state.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0, _native.last_error()
        return live


def same_bytes(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert a[3][:5].tobytes() == b[3][:5].tobytes()


def test_every_row_minus_one_is_exaspim_teasar_round_on_every_byte(dev):      # noqa: F811
    loop = Rounds(dev, case("touching"))
    for t in range(3):
        old = loop.round()
        assert old[3][5] == -1      # the old entry has five words
        new = loop.round([-1] * (loop.k + 1))
        same_bytes(new, old)
        assert new[3][5] == 0 and new[3][0] == old[3][0] >= 1, t
        assert loop.apply() == old[3][0]
    # row 0 is not read
    same_bytes(loop.round([12345] + [-1] * loop.k), loop.round())


def test_a_given_target_on_the_skeleton_is_no_branch_and_the_label_goes_on(dev):      # noqa: F811
    loop = Rounds(dev, case("touching"))
    source = int(case("touching")[1][1])
    first = loop.round([-1, source, -1])      # round 1: nothing is on the skeleton, the walk ends at the source
    assert first[0][1] == source and first[1][1] == 1 and first[2][1] == -1 and first[3][0] == 2 and first[3][3] == 2
    loop.apply()
    plain = loop.round()
    again = loop.round([-1, source, -1])      # now the source is on the skeleton
    assert (again[0][1], again[1][1], again[2][1]) == (-1, 0, -1)
    assert (again[0][2], again[1][2], again[2][2]) == (plain[0][2], plain[1][2], plain[2][2])      # label 2 as ever
    assert again[3][0] == 1 and again[3][1] == 0 and again[3][2] == plain[1][2] and again[3][5] == 0
    loop.apply()
    after = loop.round()
    assert after[0][1] >= 0 and after[1][1] >= 1 and after[3][0] >= 1      # label 1 is not finished
    # a given target that is no longer valid but not on the skeleton is walked from: the source's neighbour
    d, h, w = case("touching")[0].shape
    near = source + 1
    assert case("touching")[0].reshape(-1)[near] == 1 and not (loop.mask.reshape(-1)[near].item() & 3)
    walked = loop.round([-1, near, -1])
    assert walked[0][1] == near and walked[1][1] >= 1 and walked[2][1] == source and walked[3][0] >= 1


def test_a_refused_row_is_counted_and_read_as_minus_one(dev):      # noqa: F811
    labels = case("pieces")[0]
    loop = Rounds(dev, case("pieces"))
    n = labels.size
    far = tref.index_of(labels.shape, (3, 8, 15))      # label 1's far piece: its daf is infinite
    other = tref.index_of(labels.shape, (1, 4, 7))     # a voxel of label 4
    assert labels.reshape(-1)[far] == 1 and labels.reshape(-1)[other] == 4
    plain = loop.round()
    for given, count in (([-1, far, -1, -1, -1], 1), ([-1, other, n, -5, 0], 4), ([-1, n + 7, -1, -2**31, -1], 2),
                         ([-1, -1, -1, -1, other], 0)):
        got = loop.round(given)
        assert got[3][5] == count, given
        if count:
            same_bytes(got, plain)
    assert loop.round([-1, -1, -1, -1, other])[0][4] == other
    loop.apply()
    assert loop.round([-1, far, -1, -1, -1])[3][5] == 1      # and in a later round


def test_the_given_entry_refuses_what_the_old_one_refuses(dev):      # noqa: F811
    loop = Rounds(dev, case("y"))
    lib, rows = loop.lib, loop.k + 1
    full, out = guarded(dev, 4 * rows + 8, torch.int32)
    lengths = out[2 * rows:].view(torch.int64)[:rows]
    given = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    good = [loop.labels.data_ptr(), loop.daf.data_ptr(), loop.parents.data_ptr(), loop.hops.data_ptr(), loop.dims,
            loop.k, loop.mask.data_ptr(), given.data_ptr(), out.data_ptr(), lengths.data_ptr(),
            out[rows:].data_ptr(), loop.state.data_ptr(), loop.workspace.data_ptr(), loop.need, None]
    state_before = loop.state.cpu().numpy().tobytes()
    for at, value in ((0, None), (7, None), (8, None), (11, None), (12, None), (4, _native.int3((0, 3, 3))),
                      (5, -1), (7, given.data_ptr() + 2), (9, lengths.data_ptr() + 4), (12, loop.workspace.data_ptr() + 8)):
        args = list(good)
        args[at] = value
        assert lib.exaspim_teasar_round_given(*args) == -1, at
        assert _native.last_error().startswith("teasar_round_given:"), _native.last_error()
    args = list(good)
    args[13] = loop.need - 1
    assert lib.exaspim_teasar_round_given(*args) == -3
    torch.cuda.synchronize()
    assert bool((full.view(torch.uint8) == 0xFF).all()) and loop.state.cpu().numpy().tobytes() == state_before


# ---- 2. the loops through Python ------------------------------------------------------------------------------------
class Run:
    pass


def run_loop(dev, inputs, form, scale, const, given, max_paths=None):      # noqa: F811
    labels, sources, dbf, daf, cost = (torch.from_numpy(np.array(a)).to(dev) for a in inputs)
    field, _, _ = inference._geodesic_on_device(labels, sources, cost)
    parents, hops = inference._geodesic_parents_on_device(labels, sources, field, cost)
    boxes = inference.segment_table(labels, n_labels=len(inputs[1]) - 1, return_device_tensors=True)[1]
    states, stats = [], {}

    def on_round(t, mask):
        states.append(mask.cpu().numpy().copy())

    if form == "single":
        out = inference._teasar_on_device(labels, sources, dbf, daf, parents, hops, boxes, float(scale), float(const),
                                          max_paths, stats, on_round, targets_before=given)
    else:
        out = inference._fix_branching_on_device(labels, sources, dbf, daf, cost, field, parents, hops, boxes,
                                                 float(scale), float(const), max_paths, stats, on_round,
                                                 targets_before=given)
    run = Run()
    run.voxels, run.radii, run.before, run.offsets, run.branch_label, run.branch_round, run.branch_junction = (
        t.cpu().numpy() for t in out)
    run.states, run.stats = states, stats
    run.parents, run.hops = parents.cpu().numpy(), hops.cpu().numpy()
    return run


def oracle(inputs, form, scale, const, given, run, max_paths=None):
    labels, sources, dbf, daf, cost = inputs
    if form == "single":      # on the device's parental field, which tests/test_gpu_parents.py holds to its oracle
        return fx.single(labels, sources, dbf, daf, run.parents, run.hops, scale, const, given, max_paths=max_paths)
    return fx.loop(labels, sources, dbf, daf, cost, scale, const, given, max_paths=max_paths)


def same(got, want, form):
    assert len(got.states) == len(want.states) == got.stats["rounds"]
    for t, (a, b) in enumerate(zip(got.states, want.states)):
        np.testing.assert_array_equal(a, b, err_msg=f"the state after round {t + 1}")
    names = ("voxels", "radii", "offsets", "branch_label", "branch_round", "branch_junction")
    for name, b in zip(names, want.arrays()):
        np.testing.assert_array_equal(getattr(got, name), b, err_msg=name)
    assert got.before.tolist() == want.before
    assert got.stats["vertices"] == want.new and got.stats["live_labels"] == want.live
    assert got.stats["empty_rounds"] == want.empty
    assert got.stats["given_rounds"] == max([0] + [len(v) for v in want.given.values()])
    if form == "loop":
        rounds = got.stats["rounds"]
        assert got.stats["updates"] == max(rounds - 1 - sum(1 for t in want.empty if t < rounds), 0)


def device_targets(dev, labels, k):      # noqa: F811
    """inference.border_targets on the device, held to the brute force."""
    given = inference.border_targets(torch.from_numpy(np.array(labels)).to(dev), n_labels=k,
                                     return_device_tensors=True)
    rows = border_ref.brute_force(labels, k)
    np.testing.assert_array_equal(torch.stack(given, dim=1).cpu().numpy(), rows)
    return given, (rows[:, 0], rows[:, 1])


@pytest.mark.parametrize("form", ["single", "loop"])
@pytest.mark.parametrize("name", sorted(fx.CASES))
def test_the_state_after_every_round_with_the_border_targets_given(dev, name, form):      # noqa: F811
    inputs = case(name)
    k = len(inputs[1]) - 1
    given, rows = device_targets(dev, inputs[0], k)
    for scale, const in ((1.25, 0.0), (0.0, 2.0)):
        got = run_loop(dev, inputs, form, scale, const, given)
        want = oracle(inputs, form, scale, const, rows, got)
        same(got, want, form)
        sets = want.vertex_sets(k)
        assert all(set(v) <= sets[row] for row, v in want.given.items())
        assert got.stats["given_rounds"] >= 1 and not (got.states[-1] & tref.VALID).any()
    if name == "pieces":
        assert sum(len(v) for v in want.given.values()) < len(rows[0])      # the far piece's rows were dropped


@pytest.mark.parametrize("form", ["single", "loop"])
def test_empty_rounds_and_max_paths_inside_the_given_rounds(dev, form):      # noqa: F811
    inputs = fx.faces_comb(source_at_end=True)
    labels = inputs[0]
    spine = np.nonzero(labels.reshape(-1) == 1)[0]
    spine = spine[(spine // labels.shape[2]) % labels.shape[1] == 0]
    rows = (np.ones(2 * len(spine), dtype=np.int32), np.concatenate([spine[::-1], spine]).astype(np.int32))   # unsorted, twice
    given = tuple(torch.from_numpy(a).to(dev) for a in rows)
    full = run_loop(dev, inputs, form, 1.25, 0.0, given)
    want = oracle(inputs, form, 1.25, 0.0, rows, full)
    same(full, want, form)
    assert full.stats["given_rounds"] == len(spine) and full.stats["empty_rounds"][:3] == [2, 3, 4]
    assert full.stats["rounds"] > len(spine)      # the teeth come after the given rounds
    for max_paths in (1, 3, len(spine)):
        cut = run_loop(dev, inputs, form, 1.25, 0.0, given, max_paths=max_paths)
        same(cut, oracle(inputs, form, 1.25, 0.0, rows, cut, max_paths=max_paths), form)
        assert cut.stats["rounds"] == max_paths and cut.voxels.tolist() == full.voxels[:len(cut.voxels)].tolist()
        assert (cut.states[-1] & tref.VALID).any()


def public_inputs(dev, name):      # noqa: F811
    labels, sources, dbf, daf, cost = (np.array(a) for a in case(name))
    field = inference.geodesic_field(labels, sources, cost=cost)
    parents, hops = inference.geodesic_parents(labels, sources, field=field, cost=cost, return_hops=True)
    return labels, sources, dbf, daf, cost, field, parents, hops


def test_none_is_todays_call_and_the_public_functions_are_the_loops(dev):      # noqa: F811
    labels, sources, dbf, daf, cost, field, parents, hops = public_inputs(dev, "touching")
    kw = dict(scale=1.25, const=0.0)
    stats, none_stats = {}, {}
    today = inference.teasar_branches(labels, sources, dbf, daf, parents, hops, stats=stats, **kw)
    none = inference.teasar_branches_given(labels, sources, dbf, daf, parents, hops, None, stats=none_stats, **kw)
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(today, none))
    assert stats == none_stats and "given_rounds" not in stats
    fix_stats, fix_none = {}, {}
    today = inference.teasar_branches_fix_branching(labels, sources, dbf, daf, cost, stats=fix_stats, **kw)
    none = inference.teasar_branches_fix_branching_given(labels, sources, dbf, daf, cost, None, stats=fix_none, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(today, none))
    assert {key: v for key, v in fix_stats.items() if "sweeps" not in key} == {
        key: v for key, v in fix_none.items() if "sweeps" not in key}
    # an empty table of targets is today's result too
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(
        today, inference.teasar_branches_fix_branching_given(labels, sources, dbf, daf, cost, empty, **kw)))
    # with targets: numpy in, numpy out, and the oracle's arrays
    k = len(sources) - 1
    rows = border_ref.brute_force(labels, k)
    given = (rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32))
    got = inference.teasar_branches_fix_branching_given(labels, sources, dbf, daf, cost, given, **kw)
    want = fx.loop(labels, sources, dbf, daf, cost, 1.25, 0.0, given)
    for a, b in zip(got, want.arrays()):
        assert isinstance(a, np.ndarray)
        np.testing.assert_array_equal(a, b)
    got = inference.teasar_branches_given(labels, sources, dbf, daf, parents, hops, given, **kw)
    want = fx.single(labels, sources, dbf, daf, parents, hops, 1.25, 0.0, given)
    for a, b in zip(got, want.arrays()):
        np.testing.assert_array_equal(a, b)
    # a row of another label is refused by the kernel and raises; a label outside 1..K or a voxel outside the volume
    # is refused before
    wrong = (np.array([1], dtype=np.int32), np.array([int(np.nonzero(labels.reshape(-1) == 2)[0][0])], dtype=np.int32))
    with pytest.raises(RuntimeError, match="refused 1 given target"):
        inference.teasar_branches_given(labels, sources, dbf, daf, parents, hops, wrong, **kw)
    for bad in ((np.array([k + 1], dtype=np.int32), np.array([0], dtype=np.int32)),
                (np.array([1], dtype=np.int32), np.array([labels.size], dtype=np.int32))):
        with pytest.raises(ValueError, match="targets_before"):
            inference.teasar_branches_given(labels, sources, dbf, daf, parents, hops, bad, **kw)


def test_two_runs_give_the_same_bits(dev):      # noqa: F811
    inputs = case("thick_t")
    given, _ = device_targets(dev, inputs[0], 1)
    a = run_loop(dev, inputs, "loop", 1.25, 0.0, given)
    b = run_loop(dev, inputs, "loop", 1.25, 0.0, given)
    for name in ("voxels", "radii", "before", "offsets", "branch_label", "branch_round", "branch_junction"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert len(a.states) == len(b.states) and all(x.tobytes() == y.tobytes() for x, y in zip(a.states, b.states))
    for key in ("rounds", "reads", "vertices", "live_labels", "updates", "given_rounds", "empty_rounds"):
        assert a.stats[key] == b.stats[key], key


# ---- 3. skeletonize -------------------------------------------------------------------------------------------------
def cut_volume():
    """tests/penalty_ref.py's chain volume cut so that its labels run into the faces; the bar keeps its cavity."""
    return np.ascontiguousarray(penalty_ref.chain_volume()[2:14, 4:18, 6:36])


@pytest.mark.parametrize("fix_branching", [True, False])
def test_skeletonize_fix_borders_against_the_composed_oracles(dev, fix_branching):      # noqa: F811
    big = cut_volume()
    scale, const = 1.25, 2.0
    chain = inference._skeleton_chain_on_device(torch.from_numpy(big).to(dev), scale, const, 4, 100000.0, True, None,
                                                fix_branching, fix_borders=True)
    filled, _ = holes_ref.by_components(big)
    assert (filled != big).any()      # the targets are those of the filled labels
    np.testing.assert_array_equal(chain["labels"].cpu().numpy(), filled)
    k = int(filled.max())
    rows = border_ref.brute_force(filled, k)
    np.testing.assert_array_equal(torch.stack(chain["border_targets"], dim=1).cpu().numpy(), rows)
    dbf, roots, daf, cost = (chain[name].cpu().numpy() for name in ("dbf", "roots", "daf", "cost"))
    np.testing.assert_array_equal(dbf, tref.dbf_of(filled))
    np.testing.assert_array_equal(ref.bits(daf), ref.bits(ref.relaxation(filled, roots)))
    given = (rows[:, 0], rows[:, 1])
    if fix_branching:
        want = fx.loop(filled, roots, dbf, daf, cost, scale, const, given)
    else:
        want = fx.single(filled, roots, dbf, daf, chain["parents"].cpu().numpy(), chain["hops"].cpu().numpy(), scale,
                         const, given)
    for name, b in zip(("voxels", "radii", "offsets", "branch_label", "branch_round", "branch_junction"), want.arrays()):
        np.testing.assert_array_equal(chain[name].cpu().numpy(), b, err_msg=name)
    assert chain["before"].cpu().tolist() == want.before and len(want.states) >= 2
    skeletons = inference.skeletonize_fix_borders(big, fix_branching=fix_branching, scale=scale, const=const)
    sets = want.vertex_sets(k)
    assert sorted(skeletons) == [row for row in range(1, k + 1) if sets[row]] and len(skeletons) >= 2
    on_a_face = 0
    for row, (vertices, parent, radius) in skeletons.items():
        index = np.ravel_multi_index(tuple(vertices.T), big.shape)
        assert set(index.tolist()) == sets[row]
        assert set(want.given[row]) <= set(index.tolist())      # every eligible cut centre is a vertex
        on_a_face += len(want.given[row])
    assert on_a_face >= 4
    plain = inference.skeletonize(big, fix_branching=fix_branching, scale=scale, const=const)
    assert any(set(map(tuple, plain[row][0].tolist())) != set(map(tuple, skeletons[row][0].tolist())) for row in plain)


def test_skeletonize_is_unchanged_and_the_switch_is_a_bool(dev):      # noqa: F811
    big = cut_volume()
    kw = dict(scale=1.25, const=2.0)
    today = inference.skeletonize(big, **kw)
    off = inference.skeletonize_fix_borders(big, fix_borders=False, **kw)
    assert sorted(today) == sorted(off)
    for row in today:
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(today[row], off[row]))
    labelled = inference.skeletonize_labels(big, **kw)
    off = inference.skeletonize_fix_borders(big, fix_borders=False, fix_branching=False, **kw)
    for row in labelled:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(labelled[row], off[row]))
    for bad in (1, None, "yes"):
        with pytest.raises(TypeError, match="fix_borders must be a bool"):
            inference.skeletonize_fix_borders(big, fix_borders=bad)
