"""
Every public entry point of the Python layer with torch.empty and numpy.empty poisoned (-m gpu).

The C ABI is tested on buffers its tests fill with 0xFF themselves. The wrappers in front of it allocate their own
-- workspaces, outputs, state words, the rows of the TEASAR loop, the ping-pong graphs of the contraction rounds,
the id tables and seam planes of the stream classes, the carry pool of the sliding window, the slab drain's slots,
the host results that write_block-style callbacks fill piecewise -- with torch.empty and np.empty, and fresh device
and host pages are zero, which in the label pipeline is usually the right initial value. Here every entry point
runs with tests/poisoned_alloc.py in place: twice under 0x00 (is it bit-stable from run to run at all), then under
0xFF, 0x7F and 0x01. Every returned array must have the bits of the 0x00 run (floats through their integer view),
the 0xFF run is held to the oracle the entry point's own test file uses, and the helper's counters prove that
poison reached the code under test. Inputs are made and uploaded before the context is entered: only the
wrappers' own allocations are poisoned. tests/test_alloc_sites_cpu.py keeps every allocation of the package
visible to the helper.

A result that depends on the fill is a read of memory that nothing wrote.
"""

import numpy as np
import pytest
import torch

import components_ref
import dbf_ref
import dominant_ref
import geodesic_ref as ref
import holes_ref
import parents_ref as pref
import penalty_ref
import premerge_ref
import region_graph_ref
import teasar_ref as tref
import watershed_ref
from aind_exaspim_neuron_segmentation_amd import inference
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from poisoned_alloc import poisoned
from test_gpu_bf16x3 import make_model
from test_gpu_teasar import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7F, 0x01)
SHAPE = (12, 20, 40)      # two tiles along z and x, three along y, none of them whole


def flat(out):
    """The arrays of a result, in order: numpy arrays, downloaded tensors, numbers and lists of numbers."""
    if isinstance(out, torch.Tensor):
        return [out.detach().cpu().numpy()]
    if isinstance(out, np.ndarray):
        return [out]
    if isinstance(out, dict):
        return [a for key in sorted(out) for a in flat(out[key])]
    if isinstance(out, (tuple, list)) and any(isinstance(o, (torch.Tensor, np.ndarray, tuple, list, dict)) for o in out):
        return [a for o in out for a in flat(o)]
    return [np.asarray(out)]


def differences(a, b):
    """Which arrays of two flat results differ in shape, dtype or a single bit (floats by their bytes)."""
    if len(a) != len(b):
        return [f"{len(a)} arrays against {len(b)}"]
    found = []
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape or x.dtype != y.dtype:
            found.append(f"array {i}: {x.dtype} {x.shape} against {y.dtype} {y.shape}")
        elif np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes():
            xb = np.ascontiguousarray(x).reshape(-1).view(np.uint8).reshape(x.size, -1)
            yb = np.ascontiguousarray(y).reshape(-1).view(np.uint8).reshape(y.size, -1)
            where = np.flatnonzero((xb != yb).any(axis=1))
            found.append(f"array {i} ({x.dtype} {x.shape}): {where.size} words differ, first at flat index "
                         f"{where[:4].tolist()}: {x.reshape(-1)[where[:4]].tolist()} against "
                         f"{y.reshape(-1)[where[:4]].tolist()}")
    return found


def under_every_fill(monkeypatch, name, run, hold, host_result=False, tolerance=None, pinned=False, counted=None):
    """
    run() twice under 0x00, then under every poison; hold(result) is the oracle's check and sees the 0xFF run.
    counted(counts), if given, checks the counters of every poisoned run beyond "at least one".
    tolerance: only for an entry point that is not bit-stable from run to run (a finding, named in its test):
    max |difference| allowed between two runs instead of equal bits.
    """
    with poisoned(monkeypatch, 0x00) as counts:
        base = flat(run())
    with poisoned(monkeypatch, 0x00):
        again = flat(run())
    unstable = differences(base, again)
    if unstable and tolerance is None:
        pytest.fail(f"{name}: two runs under 0x00 differ: {unstable}")
    print(f"{name}: run-to-run bit-stable: {not unstable}; fill 0x00: {counts}")
    for fill in POISONS:
        with poisoned(monkeypatch, fill) as counts:
            out = run()
        print(f"{name}: fill {fill:#04x}: {counts}")
        assert counts.calls["device"] >= 1 and counts.bytes["device"] >= 1, f"{name}: no device allocation was poisoned"
        if host_result:
            assert counts.calls["numpy"] >= 1 and counts.bytes["numpy"] >= 1, f"{name}: no host result was poisoned"
        if pinned:      # (page-locked, or pageable where the runtime refuses to lock more memory)
            assert counts.calls["pinned"] + counts.calls["host"] >= 1, f"{name}: no staging buffer was poisoned"
        if counted is not None:
            counted(counts)
        got = flat(out)
        if unstable:
            assert len(got) == len(base)
            for x, y in zip(got, base):
                assert x.shape == y.shape and x.dtype == y.dtype
                assert np.abs(x.astype(np.float64) - y.astype(np.float64)).max(initial=0) <= tolerance, (name, hex(fill))
        else:
            found = differences(got, base)
            assert not found, f"{name}: the result depends on the fill {fill:#04x}: {found}"
        if fill == 0xFF:
            hold(out)


def equal(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_array_equal(got, want, err_msg=what)


def same_graph(got, want):
    for g, w, what in zip(got, want, ("edges", "counts", "sums", "sizes", "map")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=what)


# ---- shared inputs and oracles: made once, only read ---------------------------------------------------------
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        value = make()
        for a in flat(value) if not isinstance(value, dict) else flat(list(value.values())):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = value
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _forget():
    yield
    _CACHE.clear()


def affinities():
    return cached("aff", lambda: np.random.default_rng(5).random((3,) + SHAPE, dtype=np.float32))


def fragments_of(kind):
    """(fragments, K) of the oracle: components above 0.75, or the watershed between 0.3 and 0.7."""
    if kind == "components":
        return cached("frag c", lambda: components_ref.components(affinities(), 0.75, 0))
    return cached("frag w", lambda: watershed_ref.fragments(affinities(), 0.3, 0.7, 0))


def graph_of(kind):
    return cached("graph " + kind, lambda: region_graph_ref.region_graph(fragments_of(kind)[0], affinities(),
                                                                         fragments_of(kind)[1]))


# ---- 1. components and fragments -------------------------------------------------------------------------------
def test_affinities_to_components(dev, monkeypatch):  # noqa: F811
    aff = affinities()
    want, k = components_ref.components(aff, 0.75, 5)
    assert 0 < k < components_ref.components(aff, 0.75, 0)[1]      # the size filter removes some and keeps others
    on_device = torch.from_numpy(np.array(aff)).to(dev)

    def run():
        return (inference.affinities_to_components(np.array(aff), 0.75, 5),
                inference.affinities_to_components(on_device, 0.75, 5, return_device_tensor=True))

    def hold(out):
        equal(out[0], want)
        equal(out[1], want)

    under_every_fill(monkeypatch, "affinities_to_components", run, hold)


def test_watershed_fragments(dev, monkeypatch):  # noqa: F811
    aff = affinities()
    want, k = watershed_ref.fragments(aff, 0.3, 0.7, 3)
    assert 0 < k < watershed_ref.fragments(aff, 0.3, 0.7, 0)[1]

    def run():
        return inference.watershed_fragments(np.array(aff), 0.3, 0.7, 3)

    under_every_fill(monkeypatch, "watershed_fragments", run, lambda out: equal(out, want))


# ---- 2. the region graph and its contractions --------------------------------------------------------------------
def test_region_graph(dev, monkeypatch):  # noqa: F811
    aff = affinities()
    fragments, k = fragments_of("components")
    want = graph_of("components")
    assert len(want[0]) > 1000

    def run():
        return inference.region_graph(np.array(fragments), np.array(aff))

    under_every_fill(monkeypatch, "region_graph", run, lambda out: same_graph(out, want))


def test_premerge_region_graph(dev, monkeypatch):  # noqa: F811
    graph = premerge_ref.random_graph(31, 600, 1500, 4)
    want_graph, want_map, want_history = premerge_ref.rounds(*graph, 0.9, 20, limit=6)
    assert len(want_history) >= 3      # the third round writes into the first round's buffers, handed back as spare

    def run():
        return inference.premerge_region_graph(*(np.array(a) for a in graph), 0.9, 20, rounds=6)

    def hold(out):
        same_graph(out[:5], want_graph + (want_map,))
        assert out[5] == want_history and len(out[5]) >= 3

    under_every_fill(monkeypatch, "premerge_region_graph", run, hold)


def test_contract_dominant_edges(dev, monkeypatch):  # noqa: F811
    graph = region_graph_ref.mean_graph(31, 600, 1500)
    want_graph, want_map, want_history = dominant_ref.rounds(*graph, 0.9)
    assert len(want_history) >= 3

    def run():
        return inference.contract_dominant_edges(*(np.array(a) for a in graph), 0.9)

    def hold(out):
        same_graph(out[:5], want_graph + (want_map,))
        assert out[5] == want_history and len(out[5]) >= 3

    under_every_fill(monkeypatch, "contract_dominant_edges", run, hold)


@pytest.mark.parametrize("path", ["plain", "premerge", "device_merge"])
@pytest.mark.parametrize("kind", ["components", "watershed"])
def test_agglomerate_affinities(dev, monkeypatch, kind, path):  # noqa: F811
    aff = affinities()
    fragments, k = fragments_of(kind)
    graph = graph_of(kind)
    threshold, min_size, floor = 0.6, 10, 6
    how = dict(fragment_threshold=0.75) if kind == "components" else dict(fragments="watershed", aff_threshold_low=0.3,
                                                                          aff_threshold_high=0.7)
    more = {"plain": {}, "premerge": dict(premerge_size=floor), "device_merge": dict(device_merge_rounds=64)}[path]

    def oracle():
        if path == "premerge":
            reduced, composed, history = premerge_ref.rounds(*graph, threshold, floor, limit=4)
            assert history[0] < k
            table, s = region_graph_ref.agglomerate(*reduced, threshold, min_size)
            return table[composed][fragments].astype(np.int32)
        table, s = region_graph_ref.agglomerate(*graph, threshold, min_size)      # device rounds change no label
        return table[fragments].astype(np.int32)

    want = cached(("agglomerated", kind, path == "premerge"), oracle)
    assert 1 < int(want.max()) < k
    if path == "device_merge":
        assert len(dominant_ref.rounds(*graph, threshold)[2]) >= 3

    def run():
        return inference.agglomerate_affinities(np.array(aff), [threshold], min_size, **how, **more)

    def hold(out):
        assert out.dtype == np.int32
        equal(out, want)
        if path == "device_merge":      # and, bit for bit, the labels of the call without device rounds
            equal(out, inference.agglomerate_affinities(np.array(aff), [threshold], min_size, **how))

    under_every_fill(monkeypatch, f"agglomerate_affinities[{kind}, {path}]", run, hold)


# ---- 3. holes, distances, the table ------------------------------------------------------------------------------
def label_volume():
    """Blocky labels 1 .. 4 with enclosed cavities, background 0 and -3, and id 3 absent."""
    def make():
        rng = np.random.default_rng(77)
        labels = holes_ref.punched(rng, holes_ref.blocky(rng, SHAPE, 4), 0.15)
        labels[labels == 3] = 0
        labels[4:9, 6:13, 10:30] = 2
        labels[6, 8:11, 15:22] = 0      # a cavity that is certainly enclosed
        return np.ascontiguousarray(labels, dtype=np.int32)
    return cached("labels", make)


def test_fill_holes(dev, monkeypatch):  # noqa: F811
    labels = label_volume()
    want, stats = holes_ref.by_components(labels)
    assert stats["filled"] >= 2 and stats["voxels"] >= 21
    on_device = torch.from_numpy(np.array(labels)).to(dev)

    def run():
        return (inference.fill_holes(np.array(labels), return_counts=True),
                inference.fill_holes(on_device, return_counts=True, return_device_tensor=True))

    def hold(out):
        for filled, holes, voxels in out:
            equal(filled, want)
            assert (holes, voxels) == (stats["filled"], stats["voxels"])

    under_every_fill(monkeypatch, "fill_holes", run, hold)


@pytest.mark.parametrize("black_border", [False, True])
def test_distance_to_boundary(dev, monkeypatch, black_border):  # noqa: F811
    labels = label_volume()
    want = dbf_ref.per_label(labels, black_border)

    def run():
        return inference.distance_to_boundary(np.array(labels), black_border=black_border)

    under_every_fill(monkeypatch, f"distance_to_boundary[{black_border}]", run, lambda out: equal(out, want))


@pytest.mark.parametrize("with_dbf", [False, True])
def test_segment_table(dev, monkeypatch, with_dbf):  # noqa: F811
    labels = label_volume()
    assert not (labels == 3).any() and (labels == 4).any()      # a row in 1..K that no voxel touches
    dbf = dbf_ref.per_label(labels) if with_dbf else None
    want = dbf_ref.segment_table(labels, dbf, 6)                # and two rows above the largest id

    def run():
        return inference.segment_table(np.array(labels), None if dbf is None else np.array(dbf), n_labels=6)

    def hold(out):
        for got, expected, what in zip(out, want, ("sizes", "boxes", "peak", "peak_index")):
            equal(got, expected, what)
        assert out[0][3] == 0 and out[0][5] == 0 and out[0][6] == 0

    under_every_fill(monkeypatch, f"segment_table[dbf={with_dbf}]", run, hold)


# ---- 4. the geodesic fields ------------------------------------------------------------------------------------------
def geodesic_case(mode):
    """Blobs with four labels, label 4 without a source; in cost mode a field with every special value."""
    def make():
        labels = ref.blobs(np.random.default_rng(13), SHAPE, 4)
        sources = ref.first_voxels(labels, 4)
        assert (sources[1:] >= 0).all()
        sources[4] = -1
        cost = ref.random_cost(np.random.default_rng(14), SHAPE) if mode == "cost" else None
        field = ref.relaxation(labels, sources, cost)
        return dict(labels=labels, sources=sources, cost=cost, field=field)
    return cached("geodesic " + mode, make)


@pytest.mark.parametrize("farthest", [False, True])
@pytest.mark.parametrize("mode", ["euclid", "cost"])
def test_geodesic_field(dev, monkeypatch, mode, farthest):  # noqa: F811
    case = geodesic_case(mode)
    labels, sources, cost, want = case["labels"], case["sources"], case["cost"], case["field"]
    assert np.isinf(want[labels == 4]).all() and np.isfinite(want[labels == 1]).any()
    want_far = ref.farthest(labels, sources, want)
    seen = {}

    def run():
        stats = {}
        out = inference.geodesic_field(np.array(labels), np.array(sources), cost=None if cost is None else np.array(cost),
                                       sweeps_per_read=1, return_farthest=farthest, stats=stats)
        seen.update(stats)
        return out

    def hold(out):
        field = out[0] if farthest else out
        equal(ref.bits(field), ref.bits(want))
        if farthest:
            equal(ref.bits(out[1]), ref.bits(want_far[0]), "far_value")
            equal(out[2], want_far[1], "far_index")
            assert out[2][4] == -1 and out[1][4] == 0
        assert seen["reads"] == seen["sweeps"] + 1 >= 4      # the state word is read after every sweep

    under_every_fill(monkeypatch, f"geodesic_field[{mode}, farthest={farthest}]", run, hold)


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("mode", ["euclid", "cost"])
def test_geodesic_parents(dev, monkeypatch, mode, given):  # noqa: F811
    case = geodesic_case(mode)
    labels, sources, cost, field = case["labels"], case["sources"], case["cost"], case["field"]
    want = cached(("parents", mode), lambda: pref.jacobi(labels, sources, field, cost)[:2])

    def run():
        return inference.geodesic_parents(np.array(labels), np.array(sources), field=np.array(field) if given else None,
                                          cost=None if cost is None else np.array(cost), sweeps_per_read=1,
                                          return_hops=True)

    def hold(out):
        equal(out[0], want[0], "parents")
        equal(out[1], want[1], "hops")
        assert (out[1][labels == 4] == -1).all()

    under_every_fill(monkeypatch, f"geodesic_parents[{mode}, field given={given}]", run, hold)


def test_trace_paths(dev, monkeypatch):  # noqa: F811
    case = geodesic_case("cost")
    parents, hops = cached(("parents", "cost"), lambda: pref.jacobi(case["labels"], case["sources"], case["field"],
                                                                   case["cost"])[:2])
    reached = np.flatnonzero(hops.reshape(-1) > 0)
    source = int(case["sources"][1])
    targets = np.concatenate([[source], np.random.default_rng(21).choice(reached, 40), [source]]).astype(np.int32)
    assert hops.reshape(-1)[source] == 0
    want = pref.paths(parents, hops, targets)
    none = np.zeros(0, dtype=np.int32)
    on_device = [torch.from_numpy(np.array(a)).to(dev) for a in (parents, hops, targets)]

    def run():
        return (inference.trace_paths(np.array(parents), np.array(hops), np.array(targets)),
                inference.trace_paths(*on_device, return_device_tensors=True),
                inference.trace_paths(np.array(parents), np.array(hops), none))

    def hold(out):
        for voxels, offsets in out[:2]:
            equal(voxels, want[0], "voxels")
            equal(offsets, want[1], "offsets")
        assert want[1][1] == 1 and want[0][0] == source      # the target with hops == 0 is its own path
        assert out[2][0].shape == (0,) and out[2][1].tolist() == [0]

    under_every_fill(monkeypatch, "trace_paths", run, hold)


# ---- 5. the TEASAR loop and the chain ----------------------------------------------------------------------------------
def teasar_case():
    return cached("teasar", lambda: tref.seeded(20, shape=(24, 24, 40), max_labels=5))


@pytest.mark.parametrize("max_paths", [None, 1])
def test_teasar_branches(dev, monkeypatch, max_paths):  # noqa: F811
    inputs = teasar_case()
    want = cached(("teasar result", max_paths), lambda: tref.incremental(*inputs, 1.25, 1.0, max_paths=max_paths))
    if max_paths is None:
        assert len(want.states) >= 2
    else:
        assert (want.states[-1] & tref.VALID).any()      # the loop is cut: its else branch reads the state on its own
    on_device = [torch.from_numpy(np.array(a)).to(dev) for a in inputs]
    seen = {}

    def run():
        stats = {}
        out = (inference.teasar_branches(*(np.array(a) for a in inputs), scale=1.25, const=1.0, max_paths=max_paths,
                                         stats=stats),
               inference.teasar_branches(*on_device, scale=1.25, const=1.0, max_paths=max_paths,
                                         return_device_tensors=True))
        seen.update(stats)
        return out

    def hold(out):
        for got in out:
            for a, b, what in zip(got, want.arrays(), ("voxels", "radii", "offsets", "branch_label", "branch_round",
                                                       "branch_junction")):
                equal(a, b, what)
        assert seen["rounds"] == len(want.states) and seen["reads"] == seen["rounds"] + 1
        assert seen["vertices"] == want.new and seen["live_labels"] == want.live

    under_every_fill(monkeypatch, f"teasar_branches[max_paths={max_paths}]", run, hold)


def test_teasar_branches_without_a_valid_label(dev, monkeypatch):  # noqa: F811
    """No label has a source: the first read of the state finds live == 0, and the empty results are built."""
    labels, sources, dbf, daf, parents, hops = teasar_case()
    nothing = np.full_like(sources, -1)
    want = tref.incremental(labels, nothing, dbf, daf, parents, hops, 1.25, 1.0)
    assert want.states == [] and want.voxels == []
    seen = {}

    def run():
        stats = {}
        out = inference.teasar_branches(*(np.array(a) for a in (labels, nothing, dbf, daf, parents, hops)), scale=1.25,
                                        const=1.0, stats=stats)
        seen.update(stats)
        return out

    def hold(out):
        for a, b in zip(out, want.arrays()):
            assert a.dtype == b.dtype
            equal(a, b)
        assert out[2].tolist() == [0] and seen["rounds"] == 0 and seen["reads"] == 1

    under_every_fill(monkeypatch, "teasar_branches[no valid label]", run, hold)


def test_skeletonize_labels(dev, monkeypatch):  # noqa: F811
    """The volume of test_skeletonize_labels_against_the_oracles; the oracles are composed as there, with the device's
    penalty field (held to its own oracle in tests/test_gpu_penalty.py) as the input of the later stages."""
    big = penalty_ref.chain_volume()
    kw = dict(scale=1.25, const=2.0, pdrf_exponent=4, pdrf_scale=100000.0)
    filled, _ = holes_ref.by_components(big)
    k = int(filled.max())
    dbf = tref.dbf_of(filled)
    first = ref.first_voxels(filled, k)
    _, roots = ref.farthest(filled, first, ref.relaxation(filled, first))
    daf = ref.relaxation(filled, roots)
    on_device = torch.from_numpy(np.array(big)).to(dev)

    def run():
        skeletons = inference.skeletonize_labels(np.array(big), **kw)
        chain = inference._skeleton_chain_on_device(on_device, kw["scale"], kw["const"], 4, 100000.0, True, None)
        return [skeletons[row] for row in sorted(skeletons)], sorted(skeletons), chain

    def hold(out):
        skeletons, rows, chain = out
        equal(chain["labels"], filled)
        equal(chain["dbf"], dbf)
        equal(chain["roots"], roots)
        equal(ref.bits(chain["daf"].cpu().numpy()), ref.bits(daf))
        cost = chain["cost"].cpu().numpy()
        ratio = penalty_ref.worst_ratio(cost, penalty_ref.cost(filled, dbf, daf, k, 4, 100000.0), filled, k, 4, 100000.0)
        assert ratio <= 1.0, ratio
        parents, hops, orphans, invalid = pref.jacobi(filled, roots, ref.relaxation(filled, roots, cost), cost)
        assert (orphans, invalid) == (0, 0)
        equal(chain["parents"], parents)
        want = tref.incremental(filled, roots, dbf, daf, parents, hops, kw["scale"], kw["const"])
        for what, b in zip(("voxels", "radii", "offsets", "branch_label", "branch_round", "branch_junction"),
                           want.arrays()):
            equal(chain[what], b, what)
        assert chain["before"].cpu().tolist() == want.before and len(want.states) >= 2
        sets = want.vertex_sets(k)
        assert rows == [row for row in range(1, k + 1) if sets[row]] and len(rows) >= 2
        for row, (vertices, parent, radius) in zip(rows, skeletons):
            index = np.ravel_multi_index(tuple(vertices.T), big.shape)
            assert set(index.tolist()) == sets[row] and index[0] == roots[row] and parent[0] == -1
            equal(radius, np.sqrt(dbf.reshape(-1)[index].astype(np.float32)))
            equal(index[parent[1:]], parents.reshape(-1)[index[1:]])

    under_every_fill(monkeypatch, "skeletonize_labels", run, hold)


# ---- 6. volumes that arrive in slabs -----------------------------------------------------------------------------------
CUTS = (5, 8)      # slabs [0, 5), [5, 8), [8, 12): no cut is a multiple of the 8-plane tile but the one that has to be


BOUNDS = list(zip((0,) + CUTS, CUTS + (SHAPE[0],)))
DEPTH_5 = [(z0, min(z0 + 5, SHAPE[0])) for z0 in range(0, SHAPE[0], 5)]      # slab_depth=5: [0, 5), [5, 10), [10, 12)


def ids_needed(dev, aff, threshold, min_size, bounds):  # noqa: F811
    """The provisional ids these slabs use: the smallest id_capacity that holds them (asked from an unpoisoned run)."""
    cs = inference.ComponentsStream(SHAPE, threshold, min_size, device=dev)
    t = torch.from_numpy(np.array(aff)).to(dev)
    for z0, z1 in bounds:
        cs.push(t[:, z0:z1])
    cs.finish()
    assert 0 < cs.ids_used < aff[0].size
    return cs.ids_used


def test_the_stream_classes(dev, monkeypatch):  # noqa: F811
    aff = affinities()
    fragments, k = fragments_of("components")
    want_graph = graph_of("components")
    capacity = ids_needed(dev, aff, 0.75, 0, BOUNDS)
    t = torch.from_numpy(np.array(aff)).to(dev)
    bounds = BOUNDS
    assert len(bounds) >= 3

    def run():
        cs = inference.ComponentsStream(SHAPE, 0.75, 0, device=dev, id_capacity=capacity)
        rgs = inference.RegionGraphStream(SHAPE, device=dev, id_capacity=capacity, edge_capacity=1 << 14)
        parts = []
        for z0, z1 in bounds:
            slab = t[:, z0:z1].contiguous()
            parts.append(cs.push(slab))
            rgs.push(parts[-1], slab)
        table, count = cs.finish()
        assert cs.ids_used == capacity
        graph = rgs.finish(table, count)
        again = rgs.finish(table[: cs.ids_used + 1], count)      # finish may be called again
        labels = cs.apply(torch.cat(parts))
        return labels, count, graph, again

    def hold(out):
        labels, count, graph, again = out
        equal(labels, fragments)
        assert count == k
        same_graph(graph, want_graph)
        same_graph(again, want_graph)

    under_every_fill(monkeypatch, "ComponentsStream and RegionGraphStream", run, hold)


@pytest.mark.parametrize("resident", [True, False])
def test_affinities_to_components_streaming(dev, monkeypatch, resident):  # noqa: F811
    aff = affinities()
    want, k = components_ref.components(aff, 0.75, 5)
    capacity = ids_needed(dev, aff, 0.75, 5, DEPTH_5)

    def run():
        blocks = []
        table, count = inference.affinities_to_components_streaming(
            np.array(aff), 0.75, 5, slab_depth=5, id_capacity=capacity,
            write_block=lambda z0, z1, block: blocks.append(block.copy()))
        labels = inference.affinities_to_components_streaming(np.array(aff), 0.75, 5, slab_depth=5, id_capacity=capacity,
                                                              keep_labels_resident=resident)
        return labels, table[np.concatenate(blocks)], count, len(blocks)

    def hold(out):
        equal(out[0], want)
        equal(out[1], want)
        assert out[2] == k and out[3] == 3

    under_every_fill(monkeypatch, f"affinities_to_components_streaming[resident={resident}]", run, hold,
                     host_result=not resident)


@pytest.mark.parametrize("resident", [True, False])
def test_agglomerate_affinities_streaming(dev, monkeypatch, resident):  # noqa: F811
    aff = affinities()
    fragments, k = fragments_of("components")
    table, s = region_graph_ref.agglomerate(*graph_of("components"), 0.6, 10)
    want = table[fragments].astype(np.int32)
    capacity = ids_needed(dev, aff, 0.75, 0, DEPTH_5)

    def run():
        return inference.agglomerate_affinities_streaming(np.array(aff), [0.6], 10, fragment_threshold=0.75, slab_depth=5,
                                                          id_capacity=capacity, edge_capacity=1 << 14,
                                                          keep_labels_resident=resident)

    def hold(out):
        assert out.dtype == np.int32 and int(out.max()) == s
        equal(out, want)

    under_every_fill(monkeypatch, f"agglomerate_affinities_streaming[resident={resident}]", run, hold,
                     host_result=not resident)


# ---- 7. the network in front ---------------------------------------------------------------------------------------------
CARRY = ((90, 85, 100), dict(batch_size=3, patch_shape=(64, 64, 64), overlap=(32, 32, 32), trim=4))      # the "ragged"
SMALL = ((72, 40, 56), dict(batch_size=4, patch_shape=(32, 32, 32), overlap=(8, 8, 8), trim=4))          # golden g5's


def models(dev, dtype):  # noqa: F811
    if ("model", dtype) not in _CACHE:
        _CACHE["model", dtype] = make_model(dev, compute_dtype=dtype)[0]
    return _CACHE["model", dtype]


def forget_engine(model):
    """
    The model packs its weights (np.empty, filled by exaspim_unet_pack_weights and uploaded as it is) and allocates
    its per-stream workspaces (torch.empty) at the first forward and keeps both. Every run() starts with this, so
    that the packed image and the workspaces are allocated again under the run's own fill.
    """
    torch.cuda.synchronize()
    model._release_engine()
    model._workspace = None


def engine_was_rebuilt(model, result_bytes=0):
    """The check of the counters: the numpy counter holds the packed image next to the host results, and the model
    has an engine and a workspace again."""
    def counted(counts):
        entry = model._engines.get(model.active_dtype())
        assert entry is not None and model._workspace, "no engine was built in the poisoned run"
        packed = int(entry["packed"].numel())
        assert packed > 0 and counts.bytes["numpy"] >= packed + result_bytes, (counts.bytes["numpy"], packed, result_bytes)
        assert counts.bytes["device"] >= sum(int(ws.numel()) for ws in model._workspace.values())
    return counted


def layers_plan_no_carry(shape, kw):
    """
    The slab pipeline behind predict_streaming and the two labelling calls hands run_sliding_window one z layer of
    patches at a time. A plane is carried from one z start to a later one of the same call, and rows along y ride on
    those links, so these calls plan no carry at any geometry: carry_plan has no link within any layer.
    """
    starts = list(inference.generate_patch_starts((1, 1) + shape, kw["patch_shape"], kw["overlap"]))
    layers = sorted({s[0] for s in starts})
    for z in layers:
        layer = [s for s in starts if s[0] == z]
        if any(link is not None for link in inference.carry_plan(layer, kw["batch_size"], kw["patch_shape"], kw["overlap"])):
            return False
    return len(layers) >= 2


def test_predict_16_bit_with_the_carry_pool_live(dev, monkeypatch):  # noqa: F811
    """
    Two z slabs of patches and two rows along y at 64^3: planes are carried down z and rows along y through the
    pool that run_sliding_window allocates with torch.empty. The oracle is the one tests/test_gpu_carry_y_forward.py
    uses: the same call with nothing carried, which the 16-bit tests hold to the float64 reference.
    """
    model = models(dev, "bf16")
    shape, kw = CARRY
    starts = list(inference.generate_patch_starts((1, 1) + shape, kw["patch_shape"], kw["overlap"]))
    succ = inference.carry_plan(starts, kw["batch_size"], kw["patch_shape"], kw["overlap"])
    links, peak, level1 = inference._carry_schedule(model, succ, starts, kw["batch_size"], kw["patch_shape"], kw["overlap"],
                                                    1, dev)
    assert links is not None and any(links) and peak >= 2, "no plane is carried: the test would prove nothing"
    ylinks, _ = inference._carry_rows_schedule(links, starts, kw["batch_size"], kw["patch_shape"], kw["overlap"])
    assert any(ylinks), "no row is carried"
    assert len({s[0] for s in starts}) >= 2 and len({s[1] for s in starts}) >= 2
    host = synthetic.synth_volume(shape, seed=61)
    vol = inference.DeviceVolume.from_array(host, dev)
    monkeypatch.setattr(inference, "CARRY_Z", False)
    want = inference.predict(vol, model, verbose=False, n_streams=1, **kw)
    monkeypatch.setattr(inference, "CARRY_Z", True)

    assert layers_plan_no_carry(shape, kw)      # the host array below goes layer by layer: only the two calls on
    #                                             the device volume carry anything

    def run():
        inference.release_pinned_buffers()
        forget_engine(model)
        return (inference.predict(vol, model, verbose=False, n_streams=1, **kw),
                inference.predict(vol, model, verbose=False, n_streams=3, **kw),
                inference.predict(host, model, verbose=False, **kw))      # a host array: the slab pipeline

    def hold(out):
        for got in out:
            assert got.dtype == np.float32 and not np.isnan(got).any()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

    under_every_fill(monkeypatch, "predict[bf16, carried planes and rows]", run, hold, host_result=True, pinned=True,
                     counted=engine_was_rebuilt(model, want.nbytes))
    inference.release_pinned_buffers()


def test_predict_fp32_and_export_half(dev, monkeypatch, golden):  # noqa: F811
    """float32 plans no carry (the pool is 16-bit); the packed weights, the engine's workspaces, the outputs and the
    staging slots are poisoned all the same: the engine is built again inside every run. Held to the reference's own
    result for this volume and model (golden g5) at test_gpu_parity.py's bound."""
    model = models(dev, "fp32")
    shape, kw = SMALL
    g = golden("g5_fullwidth_small.npz")
    host = synthetic.synth_volume(shape, seed=11)
    vol = inference.DeviceVolume.from_array(host, dev)
    x = torch.from_numpy(np.random.default_rng(3).random((3, 7, 9, 33), dtype=np.float32) * 4 - 2).to(dev)

    def run():
        inference.release_pinned_buffers()
        forget_engine(model)
        return (inference.predict(host, model, verbose=False, **kw),
                inference.predict(vol, model, verbose=False, return_device_tensor=True, **kw),
                inference.predict(host, model, verbose=False, out_dtype=np.float16, **kw),
                inference.export_half(x))

    def hold(out):
        pred, on_device, half, exported = out
        assert pred.dtype == np.float32 and pred.shape == (3,) + shape
        assert np.abs(pred[:, ::2, ::2, ::2] - g["pred"]).max() < 5e-6
        assert np.array_equal(on_device.cpu().numpy().view(np.uint32), pred.view(np.uint32))
        assert half.dtype == np.float16 and np.array_equal(half.view(np.uint16), pred.astype(np.float16).view(np.uint16))
        assert np.array_equal(exported.cpu().numpy().view(np.uint16), x.cpu().numpy().astype(np.float16).view(np.uint16))

    voxels = int(np.prod(shape))
    under_every_fill(monkeypatch, "predict[fp32], export_half", run, hold, host_result=True, pinned=True,
                     counted=engine_was_rebuilt(model, 3 * voxels * 4 + 3 * voxels * 2))
    inference.release_pinned_buffers()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_streaming_calls(dev, monkeypatch, dtype):  # noqa: F811
    """
    predict_streaming, predict_components_streaming and predict_agglomerate_streaming on three z slabs of patches,
    with the staging slot capped at four planes so that more slabs are drained than there are slots (three). The oracles
    are their own tests': predict on the device-resident volume, and the CPU components and agglomeration of the
    affinities predict_streaming returns. No carry is planned here, whatever the geometry (layers_plan_no_carry):
    the carry pool is live in test_predict_16_bit_with_the_carry_pool_live alone.
    """
    model = models(dev, dtype)
    shape, kw = SMALL
    assert layers_plan_no_carry(shape, kw) and layers_plan_no_carry(*CARRY)
    host = synthetic.synth_volume(shape, seed=11)
    want = inference.predict(inference.DeviceVolume.from_array(host, dev), model, verbose=False, **kw)
    nonzero = want[want != 0]
    threshold = float(np.quantile(nonzero, 0.5))
    want_components, k = components_ref.components(want, threshold, 20)
    fragments, n_fragments = components_ref.components(want, threshold, 0)
    table, s = region_graph_ref.agglomerate(*region_graph_ref.region_graph(fragments, want, n_fragments), 0.6, 20)
    want_segments = table[fragments].astype(np.int32)
    assert k >= 1 and s >= 1
    monkeypatch.setattr(inference, "PINNED_SLOT_BYTES", 4 * 3 * shape[1] * shape[2] * 4)      # four planes

    def run():
        inference.release_pinned_buffers()
        forget_engine(model)
        blocks = []
        inference.predict_streaming(host, model, verbose=False, write_block=lambda z0, z1, b: blocks.append((z0, z1, b.copy())),
                                    **kw)
        return (inference.predict_streaming(host, model, verbose=False, **kw),
                np.concatenate([b[2] for b in blocks], axis=1), [b[:2] for b in blocks],
                inference.predict_components_streaming(host, model, threshold, 20, verbose=False,
                                                       keep_labels_resident=True, **kw),
                inference.predict_components_streaming(host, model, threshold, 20, verbose=False,
                                                       keep_labels_resident=False, **kw),
                inference.predict_agglomerate_streaming(host, model, [0.6], 20, verbose=False, fragment_threshold=threshold,
                                                        keep_labels_resident=True, **kw),
                inference.predict_agglomerate_streaming(host, model, [0.6], 20, verbose=False, fragment_threshold=threshold,
                                                        keep_labels_resident=False, **kw))

    def hold(out):
        pred, pieces, spans, resident, downloaded, segments, segments_downloaded = out
        assert np.array_equal(pred.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(pieces.view(np.uint32), want.view(np.uint32))
        assert len(spans) > inference._SlabDrain.N_SLOTS >= 3      # a staging slot is used again
        assert spans[0][0] == 0 and spans[-1][1] == shape[0]
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and max(z1 - z0 for z0, z1 in spans) <= 4
        equal(resident, want_components)
        equal(downloaded, want_components)
        equal(segments, want_segments)
        equal(segments_downloaded, want_segments)

    under_every_fill(monkeypatch, f"the streaming calls[{dtype}]", run, hold, host_result=True, pinned=True,
                     counted=engine_was_rebuilt(model, want.nbytes + 2 * want_components.nbytes))
    inference.release_pinned_buffers()
