"""
exaspim_geodesic_reseed, exaspim_geodesic_parents_begin_seeds and inference.geodesic_field_seeded /
geodesic_parents_seeded / teasar_branches_fix_branching / skeletonize on the GPU (-m gpu), against the oracles of
tests/fix_branching_ref.py (tests/test_fix_branching_ref_cpu.py holds them to each other). Fields are compared on
their bit patterns, everything else with array_equal on integers. The volumes cross every seam of the 8 x 8 x 32
tiles in z, y and x. Every run through the C ABI writes into buffers pre-filled with 0xFF bytes between guard
words that must not change. Nothing here provokes a fault: every refused call is rejected on the host before a
launch, and an invalid seed is range-checked before anything is read.
"""

import zipfile

import numpy as np
import pytest
import torch

import fix_branching_ref as fb
import geodesic_ref as ref
import holes_ref
import parents_ref as pref
import penalty_ref
import teasar_ref as tref
from aind_exaspim_neuron_segmentation_amd import _native, inference

pytestmark = pytest.mark.gpu

TILE = (8, 8, 32)      # (z, y, x) of the LDS pass
GUARD = 64             # elements around every output
SMALL, BIG = (9, 17, 40), (17, 24, 70)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def guarded(dev, n, dtype):
    """A 0xFF-filled buffer of GUARD + n + GUARD elements and the view of its n middle ones."""
    full = torch.full(((n + 2 * GUARD) * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8,
                      device=dev)
    return full, full.view(dtype)[GUARD:GUARD + n]


def intact(full, n, dtype):
    """The guard elements on both sides of a guarded() buffer still hold 0xFF bytes."""
    typed = full.view(dtype)
    return bool((typed[:GUARD].view(torch.uint8) == 0xFF).all() and (typed[GUARD + n:].view(torch.uint8) == 0xFF).all())


def seeing_tiles(shape, seeds):
    """The tiles that hold one of the (valid) seeds or see it in their halo."""
    out = set()
    for s in seeds:
        v = np.unravel_index(s, shape)
        for o in [(0, 0, 0)] + ref.OFFSETS:
            u = tuple(a + b for a, b in zip(v, o))
            if all(0 <= a < b for a, b in zip(u, shape)):
                out.add(tuple(a // b for a, b in zip(u, TILE)))
    return out


def run_field(dev, labels, k, seeds, cost=None, start=None, sweeps_per_call=4, limit=4096):
    """
    Through the C ABI into guarded, poisoned buffers: exaspim_geodesic_begin with every source -1 (or "start", a
    converged field, copied), exaspim_geodesic_reseed, sweeps until state[0] == 0.
    Returns (field, tiles flagged by the reseed, invalid seeds, sweeps launched).
    """
    lib = _native.lib()
    labels = np.array(labels, dtype=np.int32)
    seeds = np.array(seeds, dtype=np.int32).reshape(-1)
    shape, n = labels.shape, labels.size
    dims = _native.int3(shape)
    lab = torch.from_numpy(labels).to(dev)
    sds = torch.from_numpy(seeds).to(dev)
    cst = None if cost is None else torch.from_numpy(np.array(cost, dtype=np.float32)).to(dev)
    cost_ptr = None if cst is None else cst.data_ptr()
    need = lib.exaspim_geodesic_workspace_bytes(dims)
    assert need >= 32, _native.last_error()
    field_full, field = guarded(dev, n, torch.float32)
    state_full, state = guarded(dev, 2, torch.int32)
    ws_full, ws = guarded(dev, need, torch.uint8)      # GUARD = 64 bytes keeps the 16-byte alignment
    if start is None:
        nowhere = torch.full((k + 1,), -1, dtype=torch.int32, device=dev)
        rc = lib.exaspim_geodesic_begin(lab.data_ptr(), dims, nowhere.data_ptr(), k, field.data_ptr(), state.data_ptr(),
                                        ws.data_ptr(), need, None)
        assert rc == 0, _native.last_error()
        assert state.cpu().tolist() == [0, 0]
    else:
        field.copy_(torch.from_numpy(np.array(start, dtype=np.float32)).to(dev).reshape(-1))
        ws.fill_(0x5A)      # whatever an earlier pass left: the reseed clears the header and both flag arrays itself
    rc = lib.exaspim_geodesic_reseed(lab.data_ptr(), dims, k, sds.data_ptr() if len(seeds) else None, len(seeds),
                                     field.data_ptr(), state.data_ptr(), ws.data_ptr(), need, None)
    assert rc == 0, _native.last_error()
    flagged_first, invalid = state.cpu().tolist()
    flagged, launched = flagged_first, 0
    while flagged:
        assert launched < limit, "no convergence"
        rc = lib.exaspim_geodesic_sweeps(lab.data_ptr(), cost_ptr, dims, k, field.data_ptr(), sweeps_per_call,
                                         state.data_ptr(), ws.data_ptr(), need, None)
        assert rc == 0, _native.last_error()
        launched += sweeps_per_call
        flagged, still_invalid = state.cpu().tolist()
        assert still_invalid == invalid
    torch.cuda.synchronize()
    assert intact(field_full, n, torch.float32) and intact(state_full, 2, torch.int32)
    assert intact(ws_full, need, torch.uint8)
    np.testing.assert_array_equal(lab.cpu().numpy(), labels)      # the inputs are only read
    np.testing.assert_array_equal(sds.cpu().numpy(), seeds)
    return field.cpu().numpy().reshape(shape), flagged_first, invalid, launched


def run_parents(dev, labels, k, seeds, field, cost=None, sweeps_per_call=4, limit=4096):
    """begin_seeds, sweeps until state[0] == 0, finish: (parents, hops, orphans, invalid seeds)."""
    lib = _native.lib()
    labels = np.array(labels, dtype=np.int32)
    seeds = np.array(seeds, dtype=np.int32).reshape(-1)
    field = np.array(field, dtype=np.float32)
    shape, n = labels.shape, labels.size
    dims = _native.int3(shape)
    lab, sds, fld = (torch.from_numpy(a).to(dev) for a in (labels, seeds, field))
    cst = None if cost is None else torch.from_numpy(np.array(cost, dtype=np.float32)).to(dev)
    cost_ptr = None if cst is None else cst.data_ptr()
    need = lib.exaspim_geodesic_workspace_bytes(dims)
    hops_full, hops = guarded(dev, n, torch.int32)
    parents_full, parents = guarded(dev, n, torch.int32)
    state_full, state = guarded(dev, 3, torch.int32)
    ws_full, ws = guarded(dev, need, torch.uint8)
    rc = lib.exaspim_geodesic_parents_begin_seeds(lab.data_ptr(), dims, k, sds.data_ptr() if len(seeds) else None,
                                                  len(seeds), fld.data_ptr(), hops.data_ptr(), state.data_ptr(),
                                                  ws.data_ptr(), need, None)
    assert rc == 0, _native.last_error()
    flagged, invalid = state.cpu().tolist()[:2]
    launched = 0
    while flagged:
        assert launched < limit, "no convergence"
        rc = lib.exaspim_geodesic_parents_sweeps(lab.data_ptr(), cost_ptr, fld.data_ptr(), dims, k, hops.data_ptr(),
                                                 sweeps_per_call, state.data_ptr(), ws.data_ptr(), need, None)
        assert rc == 0, _native.last_error()
        launched += sweeps_per_call
        flagged = state.cpu().tolist()[0]
    rc = lib.exaspim_geodesic_parents_finish(lab.data_ptr(), cost_ptr, fld.data_ptr(), hops.data_ptr(), dims, k,
                                             parents.data_ptr(), state.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    assert state.cpu().tolist()[:2] == [0, invalid]
    orphans = int(state.cpu()[2])
    assert intact(hops_full, n, torch.int32) and intact(parents_full, n, torch.int32)
    assert intact(state_full, 3, torch.int32) and intact(ws_full, need, torch.uint8)
    assert fld.cpu().numpy().tobytes() == field.tobytes()
    return parents.cpu().numpy().reshape(shape), hops.cpu().numpy().reshape(shape), orphans, invalid


# ---- 1. the seeded field from scratch --------------------------------------------------------------------------
_SEAMS = {}


def seams_case(shape):
    """(labels, k, seeds, the invalid rows mixed in, the label without a seed): shared, and left unchanged."""
    if shape not in _SEAMS:
        labels, k = fb.tile_seams(shape)
        without = 3 if shape == SMALL else 2
        labels, seeds = fb.seam_seeds(labels, k, without)
        flat = labels.reshape(-1)
        invalid = [-1, -7, labels.size, labels.size + 5, 2**31 - 1, -2**31,
                   int(np.nonzero(flat == 0)[0][0]), int(np.nonzero(flat == k + 2)[0][0]),
                   int(np.nonzero(flat < 0)[0][0])]
        labels.setflags(write=False)
        _SEAMS[shape] = (labels, k, seeds, invalid, without)
    return _SEAMS[shape]


@pytest.mark.parametrize("mode", ["euclid", "cost"])
@pytest.mark.parametrize("shape", [SMALL, BIG], ids=["small", "big"])
def test_the_seeded_field_from_scratch_is_the_dijkstra(dev, shape, mode):
    labels, k, seeds, invalid, without = seams_case(shape)
    cost = ref.random_cost(np.random.default_rng(31), shape) if mode == "cost" else None
    assert len(set(seeds)) < len(seeds) and len(set(seeds)) >= 8      # duplicates, several per label
    per_label = np.bincount(labels.reshape(-1)[sorted(set(seeds))], minlength=k + 1)
    assert per_label[without] == 0 and per_label.max() >= 2
    mixed = seeds[:3] + invalid[:4] + seeds[3:] + invalid[4:]
    got, flagged, n_invalid, launched = run_field(dev, labels, k, mixed, cost)
    assert n_invalid == len(invalid)      # counted, and nothing was written for them (the guards, and the bits below)
    assert flagged == len(seeing_tiles(shape, seeds)) and launched >= 1
    want = fb.seeded_field(fb.Graph(labels, k, cost), seeds)
    np.testing.assert_array_equal(ref.bits(got), ref.bits(want))
    assert np.isinf(got[labels == without]).all() and np.isinf(got[labels == k + 2]).all()
    assert (ref.bits(got)[labels <= 0] == 0).all()
    assert (ref.bits(got).reshape(-1)[seeds] == 0).all()
    assert np.isfinite(got[(labels >= 1) & (labels <= k) & (labels != without)]).mean() > 0.5


def test_no_seeds(dev):
    labels, k, _, invalid, _ = seams_case(SMALL)
    got, flagged, n_invalid, launched = run_field(dev, labels, k, [])      # seeds_dev is NULL
    assert (flagged, n_invalid, launched) == (0, 0, 0)
    np.testing.assert_array_equal(ref.bits(got), ref.bits(np.where(labels > 0, np.float32(np.inf), np.float32(0))))
    got, flagged, n_invalid, _ = run_field(dev, labels, k, invalid)      # nothing but invalid rows
    assert (flagged, n_invalid) == (0, len(invalid))
    np.testing.assert_array_equal(ref.bits(got), ref.bits(np.where(labels > 0, np.float32(np.inf), np.float32(0))))
    parents, hops, orphans, n_invalid = run_parents(dev, labels, k, [], got)
    assert (orphans, n_invalid) == (0, 0) and (parents == -1).all() and (hops == -1).all()


# ---- 2. incremental == from scratch ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(20)))
def test_a_reseeded_field_is_the_field_from_scratch(dev, seed):
    labels, k, cost = fb.absorbing(seed, SMALL if seed % 4 else (10, 9, 66))
    rng = np.random.default_rng(300 + seed)
    first, more = fb.random_seeds(rng, labels, k, 1 + seed % 3), fb.random_seeds(rng, labels, k, 2 + seed % 2)
    if seed % 5 == 0:
        more = more + first[:1]      # a seed that is one already
    for special in (0.0, np.inf):
        assert (cost == special).any()
    assert np.isnan(cost).any() and (cost < 0).any() and (cost == np.float32(1e-3)).any() and (cost > 1e6).any()
    old, _, invalid, _ = run_field(dev, labels, k, first, cost)
    assert invalid == 0
    kept = old.copy()
    both, _, invalid, _ = run_field(dev, labels, k, more, cost, start=old)
    assert invalid == 0 and old.tobytes() == kept.tobytes()      # the caller's field is unchanged
    scratch, _, _, _ = run_field(dev, labels, k, first + more, cost)
    np.testing.assert_array_equal(ref.bits(both), ref.bits(scratch))
    np.testing.assert_array_equal(ref.bits(both), ref.bits(fb.seeded_field(fb.Graph(labels, k, cost), first + more)))
    assert (ref.bits(both) != ref.bits(old)).any() or not more


def test_the_python_layer_is_incremental_on_a_copy(dev):
    labels, k, cost = fb.absorbing(3)
    rng = np.random.default_rng(77)
    first, more = fb.random_seeds(rng, labels, k, 1), fb.random_seeds(rng, labels, k, 2)
    as_array = lambda s: np.array(s, dtype=np.int32)      # noqa: E731
    old = inference.geodesic_field_seeded(labels, as_array(first), cost=cost)
    graph = fb.Graph(labels, k, cost)
    np.testing.assert_array_equal(ref.bits(old), ref.bits(fb.seeded_field(graph, first)))
    on_device = torch.from_numpy(old).to(dev)
    stats = {}
    both = inference.geodesic_field_seeded(torch.from_numpy(labels).to(dev), torch.from_numpy(as_array(more)).to(dev),
                                           cost=torch.from_numpy(cost).to(dev), field=on_device, n_labels=k,
                                           return_device_tensor=True, stats=stats)
    assert both.data_ptr() != on_device.data_ptr() and on_device.cpu().numpy().tobytes() == old.tobytes()
    want = fb.seeded_field(graph, first + more)
    np.testing.assert_array_equal(ref.bits(both.cpu().numpy()), ref.bits(want))
    assert stats["sweeps"] >= 1 and stats["tiles_flagged"][-1] == 0
    parents, hops = inference.geodesic_parents_seeded(labels, as_array(first + more), want, cost=cost, return_hops=True)
    want_parents, want_hops, orphans, invalid = fb.seeded_parents(graph, first + more, want)
    assert (orphans, invalid) == (0, 0)
    np.testing.assert_array_equal(parents, want_parents)
    np.testing.assert_array_equal(hops, want_hops)
    with pytest.raises(ValueError, match="2 seed"):
        inference.geodesic_field_seeded(labels, as_array(first + [-1, labels.size]), cost=cost)
    with pytest.raises(ValueError, match="field of 0"):      # the field of fewer seeds: a seed's word is not +0.0
        inference.geodesic_parents_seeded(labels, as_array(first + more), old, cost=cost)
    with pytest.raises(ValueError, match="no tight predecessor"):      # the field of another cost
        inference.geodesic_parents_seeded(labels, as_array(first + more), want,
                                          cost=(cost * np.float32(2)).astype(np.float32))


def test_max_sweeps_cuts_the_seeded_sweep_loop(dev):
    """The serpentine of test_gpu_geodesic.py: eight rows, one after another, so the two tiles take turns."""
    labels = ref.serpentine()
    assert labels.shape == (16, 16, 64)
    seeds = np.array([3 * 16 * 64], dtype=np.int32)      # (3, 0, 0), the source there
    stats = {}
    want = inference.geodesic_field_seeded(labels, seeds, n_labels=1, sweeps_per_read=1, stats=stats)
    print(f"seeded serpentine: {stats}")
    assert stats["sweeps"] > 3 and stats["sweeps"] == stats["reads"] - 1 and stats["tiles_flagged"][-1] == 0
    with pytest.raises(RuntimeError, match=r"^geodesic_field_seeded: not converged after 3 sweeps"):
        inference.geodesic_field_seeded(labels, seeds, n_labels=1, sweeps_per_read=2, max_sweeps=3)
    clipped = {}
    got = inference.geodesic_field_seeded(labels, seeds, n_labels=1, sweeps_per_read=7, max_sweeps=stats["sweeps"],
                                          stats=clipped)
    assert clipped["sweeps"] == stats["sweeps"] and clipped["tiles_flagged"][-1] == 0      # 7, 7, ... and the rest
    assert clipped["reads"] == 1 + -(-stats["sweeps"] // 7)
    np.testing.assert_array_equal(ref.bits(got), ref.bits(want))


# ---- 3. seeded hops and parents ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["euclid", "cost"])
@pytest.mark.parametrize("shape", [SMALL, BIG], ids=["small", "big"])
def test_seeded_hops_and_parents_are_the_oracles(dev, shape, mode):
    labels, k, seeds, invalid, without = seams_case(shape)
    cost = ref.random_cost(np.random.default_rng(31), shape) if mode == "cost" else None
    graph = fb.Graph(labels, k, cost)
    field = fb.seeded_field(graph, seeds)
    want_parents, want_hops, orphans, n_invalid = fb.seeded_parents(graph, seeds, field)
    assert (orphans, n_invalid) == (0, 0)
    flat = field.reshape(-1)
    away = int(np.nonzero(np.isfinite(flat) & (flat > 0))[0][5])      # a seed whose field word is not +0.0
    mixed = seeds[:2] + invalid + [away] + seeds[2:]
    parents, hops, orphans, n_invalid = run_parents(dev, labels, k, mixed, field, cost)
    assert orphans == 0 and n_invalid == len(invalid) + 1
    np.testing.assert_array_equal(hops, want_hops)
    np.testing.assert_array_equal(parents, want_parents)
    index = np.arange(labels.size)
    assert sorted(index[parents.reshape(-1) == index].tolist()) == sorted(set(seeds))      # the self-parents
    assert (hops.reshape(-1)[seeds] == 0).all() and hops.max() >= 8


@pytest.mark.parametrize("seed", [1, 4, 8, 13])
def test_seeded_parents_where_costs_are_absorbed(dev, seed):
    labels, k, cost = fb.absorbing(seed)
    seeds = fb.random_seeds(np.random.default_rng(500 + seed), labels, k, 3)
    graph = fb.Graph(labels, k, cost)
    field, _, _, _ = run_field(dev, labels, k, seeds, cost)
    want_parents, want_hops, orphans, invalid = fb.seeded_parents(graph, seeds, field)
    parents, hops, got_orphans, got_invalid = run_parents(dev, labels, k, seeds, field, cost)
    assert (orphans, invalid, got_orphans, got_invalid) == (0, 0, 0, 0)
    np.testing.assert_array_equal(hops, want_hops)
    np.testing.assert_array_equal(parents, want_parents)


# ---- 4. refusals -------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_alone(dev):
    lib = _native.lib()
    labels_host, k, seeds_host, _, _ = seams_case(SMALL)
    shape, n = labels_host.shape, labels_host.size
    labels = torch.from_numpy(np.array(labels_host)).to(dev)
    seeds = torch.tensor(seeds_host, dtype=torch.int32, device=dev)
    field = torch.full((n,), 12345.0, dtype=torch.float32, device=dev)
    hops = torch.full((n,), -1234567, dtype=torch.int32, device=dev)
    state = torch.full((3,), -7654321, dtype=torch.int32, device=dev)
    need = lib.exaspim_geodesic_workspace_bytes(_native.int3(shape))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    dims = _native.int3(shape)
    calls = {
        "reseed": (lib.exaspim_geodesic_reseed,
                   ["labels", "dims", "k", "seeds", "n_seeds", "field", "state", "ws", "need", "stream"],
                   lambda: [labels.data_ptr(), dims, k, seeds.data_ptr(), len(seeds_host), field.data_ptr(),
                            state.data_ptr(), ws.data_ptr(), need, None]),
        "begin": (lib.exaspim_geodesic_parents_begin_seeds,
                  ["labels", "dims", "k", "seeds", "n_seeds", "field", "hops", "state", "ws", "need", "stream"],
                  lambda: [labels.data_ptr(), dims, k, seeds.data_ptr(), len(seeds_host), field.data_ptr(),
                           hops.data_ptr(), state.data_ptr(), ws.data_ptr(), need, None]),
    }

    def refused(which, code, what, **changes):
        fn, names, make = calls[which]
        args = make()
        for name, new in changes.items():
            args[names.index(name)] = new
        rc = fn(*args)
        torch.cuda.synchronize()
        assert rc == code, (which, changes, _native.last_error())
        assert what in _native.last_error(), (which, changes, _native.last_error())
        assert (field == 12345.0).all() and (hops == -1234567).all() and (state == -7654321).all(), (which, changes)
        assert (ws == 0xFF).all(), (which, changes)

    for which, pointers in (("reseed", ("labels", "seeds", "field", "state", "ws")),
                            ("begin", ("labels", "seeds", "field", "hops", "state", "ws"))):
        for name in pointers:
            refused(which, -1, "NULL", **{name: None})
        refused(which, -1, "dims", dims=_native.int3((9, 0, 40)))
        refused(which, -1, "dims", dims=_native.int3((9, -17, 40)))
        refused(which, -1, "dims", dims=_native.int3((2048, 1024, 1024)))      # 2^31 voxels
        refused(which, -1, "n_labels", k=-1)
        refused(which, -1, "n_seeds", n_seeds=-1)
        refused(which, -1, "n_seeds", n_seeds=-2**40)
        for name, tensor in (("labels", labels), ("seeds", seeds), ("field", field), ("state", state)):
            refused(which, -1, "misaligned", **{name: tensor.data_ptr() + 2})
        refused(which, -1, "misaligned", ws=ws.data_ptr() + 8)
        refused(which, -3, "workspace", need=need - 1)
        refused(which, -3, "workspace", need=0)
    refused("begin", -1, "misaligned", hops=hops.data_ptr() + 1)


# ---- 5. the loop -------------------------------------------------------------------------------------------------
class Run:
    """What one device run leaves, in tests/teasar_ref.py's Result's terms."""


def run_loop(dev, inputs, scale, const, max_paths=None, given=True):
    """
    inference._fix_branching_on_device with a copy of the state volume taken after every round; field, parents
    and hops of (labels, sources, cost) from the device, and held to be unchanged afterwards.
    """
    labels, sources, dbf, daf, cost = (torch.from_numpy(np.array(a)).to(dev) for a in inputs)
    field, _, _ = inference._geodesic_on_device(labels, sources, cost)
    parents, hops = inference._geodesic_parents_on_device(labels, sources, field, cost)
    kept = [t.clone() for t in (field, parents, hops, daf, cost)]
    boxes = inference.segment_table(labels, n_labels=len(inputs[1]) - 1, return_device_tensors=True)[1]
    states, stats = [], {}
    out = inference._fix_branching_on_device(labels, sources, dbf, daf, cost, field, parents, hops, boxes, float(scale),
                                             float(const), max_paths, stats,
                                             lambda t, mask: states.append(mask.cpu().numpy().copy()))
    for before, after in zip(kept, (field, parents, hops, daf, cost)):
        assert before.cpu().numpy().tobytes() == after.cpu().numpy().tobytes()      # never modified
    run = Run()
    run.voxels, run.radii, run.before, run.offsets, run.branch_label, run.branch_round, run.branch_junction = (
        t.cpu().numpy() for t in out)
    run.states, run.stats = states, stats
    return run


def same(got, want):
    assert len(got.states) == len(want.states) == got.stats["rounds"]
    for t, (a, b) in enumerate(zip(got.states, want.states)):
        np.testing.assert_array_equal(a, b, err_msg=f"the state after round {t + 1}")
    names = ("voxels", "radii", "offsets", "branch_label", "branch_round", "branch_junction")
    for name, b in zip(names, want.arrays()):
        np.testing.assert_array_equal(getattr(got, name), b, err_msg=name)
    assert got.before.tolist() == want.before
    assert got.stats["vertices"] == want.new and got.stats["live_labels"] == want.live
    assert got.stats["updates"] == max(got.stats["rounds"] - 1, 0)
    assert len(got.stats["field_sweeps"]) == len(got.stats["hops_sweeps"]) == got.stats["updates"]
    assert all(s >= 1 for s in got.stats["field_sweeps"] + got.stats["hops_sweeps"])


def check_loop(dev, inputs, scale, const, **kw):
    want = fb.loop(*inputs, scale, const, **kw)
    got = run_loop(dev, inputs, scale, const, **kw)
    same(got, want)
    return got, want


_SHAPES = {
    "y": lambda: fb.with_cost(tref.y_shape()),
    "comb": lambda: fb.with_cost(tref.comb()),
    "cross": lambda: fb.with_cost(tref.cross()),      # the tips' daf bits tie
    "touching": fb.touching,
    "pieces": lambda: fb.from_labels(penalty_ref.pieces()),
    "dots": lambda: fb.from_labels(penalty_ref.dots_and_a_line()),      # one-voxel labels
    "absent": lambda: fb.from_labels(penalty_ref.absent_ids()),
    "plane": lambda: fb.from_labels(penalty_ref.one_plane()),
    "thick_t": fb.thick_t,
}
_INPUTS = {}


def shape_case(name):
    """The shared case, left unchanged."""
    if name not in _INPUTS:
        inputs = _SHAPES[name]()
        for a in inputs:
            a.setflags(write=False)
        _INPUTS[name] = inputs
    return _INPUTS[name]


def copies(name):
    """Writable copies of a shared case, for the public entry points (torch refuses to wrap a read-only array)."""
    return tuple(np.array(a) for a in shape_case(name))


@pytest.mark.parametrize("name", list(_SHAPES))
def test_the_loop_against_the_oracle_after_every_round(dev, name):
    inputs = shape_case(name)
    rounds = []
    # the thick blocks of "pieces" need small radii to have more than one path
    for scale, const in ((1.25, 0.0), (0.5, 0.0) if name == "pieces" else (0.5, 1.0), (0.0, 3.0)):
        got, _ = check_loop(dev, inputs, scale, const)
        rounds.append(got.stats["rounds"])
    if name != "dots":      # one-voxel labels and a line from its end: one path each
        assert max(rounds) >= 2, rounds      # there was an update to check


def test_on_the_thick_t_the_device_differs_from_the_single_field_form_too(dev):
    inputs = shape_case("thick_t")
    got, want = check_loop(dev, inputs, 1.25, 0.0)
    labels, sources, dbf, daf, cost = copies("thick_t")
    field = inference.geodesic_field(labels, sources, cost=cost)
    parents, hops = inference.geodesic_parents(labels, sources, field=field, cost=cost, return_hops=True)
    single = inference.teasar_branches(labels, sources, dbf, daf, parents, hops, scale=1.25, const=0.0)
    np.testing.assert_array_equal(single[0], np.array(fb.single_field(*inputs, 1.25, 0.0).voxels, dtype=np.int32))
    assert got.voxels.tolist() != single[0].tolist() and set(got.voxels.tolist()) != set(single[0].tolist())
    assert got.branch_junction.tolist() != single[5].tolist()


@pytest.mark.parametrize("seed", [0, 1, 7, 15, 19, 24])
def test_the_loop_on_seeded_volumes(dev, seed):
    from test_teasar_ref_cpu import PARAMS

    inputs = fb.seeded(seed)
    scale, const = PARAMS[seed % len(PARAMS)]
    check_loop(dev, inputs, scale, const)


@pytest.mark.parametrize("name", ["comb", "touching", "absent", "plane"])
def test_with_one_path_per_label_it_is_teasar_branches_bit_for_bit(dev, name):
    labels, sources, dbf, daf, cost = copies(name)
    field = inference.geodesic_field(labels, sources, cost=cost)
    parents, hops = inference.geodesic_parents(labels, sources, field=field, cost=cost, return_hops=True)
    stats, fix_stats = {}, {}
    single = inference.teasar_branches(labels, sources, dbf, daf, parents, hops, scale=1.25, const=450.0, stats=stats)
    fixed = inference.teasar_branches_fix_branching(labels, sources, dbf, daf, cost, scale=1.25, const=450.0,
                                                    field=field, parents=parents, hops=hops, stats=fix_stats)
    assert len(single) == len(fixed) == 6
    for a, b in zip(single, fixed):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert stats["rounds"] == fix_stats["rounds"] == 1
    assert fix_stats["updates"] == 0 and fix_stats["field_sweeps"] == [] and fix_stats["hops_sweeps"] == []
    assert fix_stats["reads"] == stats["reads"]      # the round that does not exist costs its one target pass
    computed = inference.teasar_branches_fix_branching(labels, sources, dbf, daf, cost, scale=1.25, const=450.0)
    for a, b in zip(fixed, computed):      # field, parents and hops computed here
        assert a.tobytes() == b.tobytes()


def test_updates_are_rounds_minus_one_and_max_paths_cuts_the_loop(dev):
    inputs = shape_case("comb")
    full, want = check_loop(dev, inputs, 0.5, 1.0)
    assert full.stats["rounds"] >= 4 and full.stats["updates"] == full.stats["rounds"] - 1
    for max_paths in (1, 2, 3):
        cut, _ = check_loop(dev, inputs, 0.5, 1.0, max_paths=max_paths)
        assert cut.stats["rounds"] == max_paths and cut.stats["updates"] == max_paths - 1
        n = int(cut.offsets[-1])
        np.testing.assert_array_equal(cut.voxels, full.voxels[:n])
        assert (cut.states[-1] & tref.VALID).any()
    labels, sources, dbf, daf, cost = copies("comb")
    stats = {}
    public = inference.teasar_branches_fix_branching(labels, sources, dbf, daf, cost, scale=0.5, const=1.0, max_paths=2,
                                                     stats=stats)
    assert stats["rounds"] == 2 and stats["updates"] == 1
    np.testing.assert_array_equal(public[0], full.voxels[:len(public[0])])


def test_two_runs_give_the_same_bits(dev):
    inputs = shape_case("plane")
    a = run_loop(dev, inputs, 0.5, 1.0)
    b = run_loop(dev, inputs, 0.5, 1.0)
    for name in ("voxels", "radii", "before", "offsets", "branch_label", "branch_round", "branch_junction"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert len(a.states) == len(b.states) and all(x.tobytes() == y.tobytes() for x, y in zip(a.states, b.states))
    for key in ("rounds", "reads", "vertices", "live_labels", "updates"):      # (sweeps depend on the schedule)
        assert a.stats[key] == b.stats[key], key


def test_euclidean_steps_in_place_of_a_cost(dev):
    labels, sources, dbf, daf, _ = copies("y")
    want = fb.loop(labels, sources, dbf, daf, None, 0.0, 2.0)
    got = inference.teasar_branches_fix_branching(labels, sources, dbf, daf, None, scale=0.0, const=2.0)
    for a, b in zip(got, want.arrays()):
        np.testing.assert_array_equal(a, b)
    assert len(want.states) >= 2


# ---- 6. skeletonize ----------------------------------------------------------------------------------------------
def composed(dev, big, scale, const, fix_branching):
    """The chain on the device, its stages held to their oracles, and the loop's oracle on the device's cost."""
    chain = inference._skeleton_chain_on_device(torch.from_numpy(big).to(dev), scale, const, 4, 100000.0, True, None,
                                                fix_branching)
    filled, _ = holes_ref.by_components(big)
    np.testing.assert_array_equal(chain["labels"].cpu().numpy(), filled)
    k = int(filled.max())
    dbf = tref.dbf_of(filled)
    np.testing.assert_array_equal(chain["dbf"].cpu().numpy(), dbf)
    first = ref.first_voxels(filled, k)
    _, roots = ref.farthest(filled, first, ref.relaxation(filled, first))
    np.testing.assert_array_equal(chain["roots"].cpu().numpy(), roots)
    daf = ref.relaxation(filled, roots)
    np.testing.assert_array_equal(ref.bits(chain["daf"].cpu().numpy()), ref.bits(daf))
    cost = chain["cost"].cpu().numpy()      # an input of what follows; tests/test_gpu_penalty.py holds it to its oracle
    if fix_branching:
        want = fb.loop(filled, roots, dbf, daf, cost, scale, const)
    else:
        want = fb.single_field(filled, roots, dbf, daf, cost, scale, const)
    for name, b in zip(("voxels", "radii", "offsets", "branch_label", "branch_round", "branch_junction"), want.arrays()):
        np.testing.assert_array_equal(chain[name].cpu().numpy(), b, err_msg=name)
    assert chain["before"].cpu().tolist() == want.before and len(want.states) >= 2
    return want, filled, dbf, roots, k


@pytest.mark.parametrize("fix_branching", [True, False])
def test_skeletonize_against_the_composed_oracles(dev, fix_branching):
    big = penalty_ref.chain_volume()
    kw = dict(scale=1.25, const=2.0)
    want, filled, dbf, roots, k = composed(dev, big, kw["scale"], kw["const"], fix_branching)
    skeletons = inference.skeletonize(big, fix_branching=fix_branching, **kw)
    sets = want.vertex_sets(k)
    assert sorted(skeletons) == [row for row in range(1, k + 1) if sets[row]] and len(skeletons) >= 2
    before = dict(zip(want.voxels, want.before))
    for row, (vertices, parent, radius) in skeletons.items():
        assert vertices.dtype == np.int32 and parent.dtype == np.int32 and radius.dtype == np.float32
        index = np.ravel_multi_index(tuple(vertices.T), big.shape)
        assert set(index.tolist()) == sets[row] and (filled.reshape(-1)[index] == row).all()
        np.testing.assert_array_equal(radius, np.sqrt(dbf.reshape(-1)[index].astype(np.float32)))
        assert np.nonzero(parent < 0)[0].tolist() == [0] and index[0] == roots[row]
        rest = np.nonzero(parent >= 0)[0]
        assert index[parent[rest]].tolist() == [before[int(v)] for v in index[rest]]      # the vertex before each
    if not fix_branching:
        labelled = inference.skeletonize_labels(big, **kw)
        assert sorted(labelled) == sorted(skeletons)
        for row in skeletons:
            for a, b in zip(skeletons[row], labelled[row]):
                assert a.tobytes() == b.tobytes()


def test_the_zip_round_trip_from_device_labels(dev, tmp_path):
    big = penalty_ref.absent_ids()
    on_device = torch.from_numpy(big).to(dev)
    skeletons = inference.skeletonize(on_device)      # the reference's parameters: one path per label here
    assert sorted(skeletons) == [1, 3, 6]
    path = tmp_path / "skeletons.zip"
    inference.segmentation_to_zipped_swcs(on_device, path)
    with zipfile.ZipFile(path) as archive:
        assert sorted(archive.namelist()) == ["1.swc", "3.swc", "6.swc"]
        for row, skeleton in skeletons.items():
            text = archive.read(f"{row}.swc").decode()
            assert text == inference.skeleton_to_swc(*skeleton)
            rows = [line.split() for line in text.splitlines()]
            np.testing.assert_array_equal(np.array([[float(c) for c in r[2:5]] for r in rows]), skeleton[0])
            assert [int(r[6]) for r in rows] == [p + 1 if p >= 0 else -1 for p in skeleton[1].tolist()]
    img = inference.voxelize_skeletons(skeletons, big.shape)
    filled, _ = holes_ref.by_components(big)
    assert (img[img > 0] == filled[img > 0]).all()
    assert int((img > 0).sum()) == sum(len(s[0]) for s in skeletons.values())
    assert np.array_equal(on_device.cpu().numpy(), big)
