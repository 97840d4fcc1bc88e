"""The second level's carried planes, host side only: the plane-range rule against a brute-force statement of
it, the launcher's answer to "which tile depth, if any", the buffer budget (first level first) and the links
inference._carry_schedule hands run_sliding_window."""

import ctypes

import pytest

import layer_ref as R
from carry_ref import _brute_force, _Model
from aind_exaspim_neuron_segmentation_amd import _native, inference


@pytest.fixture(scope="module")
def probe():
    import __graft_entry__

    __graft_entry__.build()
    lib = ctypes.CDLL(R.PROBE_PATH)
    i32 = ctypes.c_int32
    lib.probe_carry1_span.restype = None
    lib.probe_carry1_span.argtypes = [i32, i32, i32, ctypes.POINTER(i32)]
    lib.probe_conv_carry_tile_depth.restype = i32
    lib.probe_conv_carry_tile_depth.argtypes = [i32, i32, i32, i32, i32, i32, i32, ctypes.c_size_t]
    return lib


def test_plane_range_is_the_brute_force_rule(probe):
    # the tile depth the launcher reports for the level-1 layers (down1.0: 32 -> 64, down1.3: 64 -> 64; the split-K
    # scratch forward() offers) -- one depth, whatever the patch
    depths = set()
    for d, h, w in ((48, 16, 64), (64, 32, 96), (96, 96, 96), (32, 16, 64)):
        scratch = (d + 2) * (h + 2) * (w + 2) * 4
        for dt in (_native.DT_F16, _native.DT_BF16):
            for ca in (32, 64):
                depths.add(probe.probe_conv_carry_tile_depth(dt, ca, 64, 16, d // 2, h // 2, w // 2, scratch))
    assert depths == {4}
    out = (ctypes.c_int32 * 2)()
    nonempty = 0
    for tz in sorted(depths):
        for d in range(16, 209, 16):
            for shift in range(1, d + 2):
                probe.probe_carry1_span(tz, d, shift, out)
                assert tuple(out) == _brute_force(tz, d, shift), (tz, d, shift)
                nonempty += out[1] > out[0]
    assert nonempty > 100
    for (d, shift), want in {(96, 64): (4, 12), (48, 16): (4, 12), (48, 24): (4, 8), (64, 32): (4, 12),
                             (32, 16): (0, 0)}.items():
        probe.probe_carry1_span(4, d, shift, out)
        assert tuple(out) == want, (d, shift)
    probe.probe_carry1_span(0, 96, 64, out)      # the layers run no configuration that carries
    assert tuple(out) == (0, 0)


def test_the_launcher_names_the_configurations_that_carry(probe):
    f16, f32, x3 = _native.DT_F16, _native.DT_F32, _native.DT_BF16X3
    depth = probe.probe_conv_carry_tile_depth
    assert depth(f16, 64, 64, 16, 48, 48, 48, 0) == 4
    assert depth(f32, 64, 64, 16, 48, 48, 48, 0) == 0 and depth(x3, 64, 64, 16, 48, 48, 48, 0) == 0
    assert depth(f16, 32, 32, 16, 48, 48, 48, 0) == 0       # a 32-cout slice: the z-column kernel
    assert depth(f16, 64, 64, 16, 48, 48, 24, 0) == 0       # 24-wide rows: another tile
    assert depth(f16, 64, 64, 16, 24, 8, 32, 0) == 4
    # the same layer with scratch for two ranges is split (12 tiles x 16 patches on 512 slots): no carry
    assert depth(f16, 64, 64, 16, 24, 8, 32, 2 * 24 * 8 * 32 * 64 * 4) == 0
    assert depth(f16, 64, 64, 16, 24, 8, 32, 50 * 18 * 66 * 4) == 4     # what forward() offers: too little to split


def test_budget_takes_the_first_level_first():
    gib = 1 << 30
    budget = inference._carry_budget
    pair, triple = 1020 << 20, 480 << 20        # about the bench's 0.95 and 0.45 GiB per batch of 16
    assert budget(17, pair, triple, 200 * gib, 36 * gib) == (True, True)
    assert budget(20, pair, triple, 200 * gib, 36 * gib) == (True, True)       # three streams
    assert budget(20, pair, triple, 200 * gib, 24 * gib) == (True, False)      # the cap holds the pairs only
    assert budget(20, pair, triple, 50 * gib, 36 * gib) == (True, False)       # half of the free memory does
    assert budget(20, pair, triple, 30 * gib, 36 * gib) == (False, False)
    assert budget(20, pair, triple, 200 * gib, 1 << 10) == (False, False)
    assert budget(20, pair, 0, 200 * gib, 36 * gib) == (True, False)           # nothing to carry at level 1
    assert budget(0, pair, triple, 200 * gib, 36 * gib) == (False, False)
    # exactly at the bound
    assert budget(4, 10, 5, 1000, 60) == (True, True) and budget(4, 10, 5, 1000, 59) == (True, False)
    assert budget(4, 10, 5, 118, 1000) == (True, False) and budget(4, 10, 5, 120, 1000) == (True, True)
    assert budget(4, 10, 5, 79, 1000) == (False, False)


# (volume, patch, overlap, batch size, a link's level-1 range)
PLANS = {
    "bench": ((1024, 1024, 1024), (96, 96, 96), (32, 32, 32), 16, (4, 12)),
    "48 deep, shift 24": ((120, 32, 96), (48, 32, 64), (24, 8, 32), 2, (4, 8)),
    "32 deep: level 0 only": ((64, 16, 96), (32, 16, 64), (16, 8, 32), 2, (0, 0)),
    "one slab": ((96, 224, 352), (96, 96, 96), (32, 32, 32), 5, None),
}


def _schedule(name, monkeypatch, level1=True, cap=None, free=1 << 50, switch=True, n_streams=1):
    shape, patch, overlap, batch_size, _ = PLANS[name]
    starts = list(inference.generate_patch_starts((1, 1) + shape, patch, overlap))
    succ = inference.carry_plan(starts, batch_size, patch, overlap)
    monkeypatch.setattr(inference, "CARRY_Z1", switch)
    if cap is not None:
        monkeypatch.setattr(inference, "CARRY_POOL_BYTES", cap)
    model = _Model(level1)
    got = inference._carry_schedule(model, succ, starts, batch_size, patch, overlap, n_streams, None, free=free)
    pair = 2 * sum(model.carry_pair_elems((batch_size,) + patch))
    triple = 2 * sum(model.carry_triple_elems((batch_size,) + patch))
    return succ, got, pair, triple


@pytest.mark.parametrize("name", list(PLANS))
def test_a_triple_goes_with_a_pair_exactly_where_the_range_is_not_empty(name, monkeypatch):
    want1 = PLANS[name][4]
    succ, (links, peak, level1), pair, triple = _schedule(name, monkeypatch, cap=1 << 50)
    if want1 is None:
        assert (links, peak, level1) == (None, 0, False) and set(succ) == {None}
        return
    assert [None if l is None else l[0] for l in links] == succ     # every link of the plan takes a pair
    assert level1 == (want1 != (0, 0))
    assert all(l[3] == want1 for l in links if l is not None)
    assert all(l[2][1] > l[2][0] for l in links if l is not None)
    # CARRY_Z1 off, or an engine that gives no level-1 range: the same links and sets, pairs only
    for kw in (dict(switch=False), dict(level1=False)):
        _, (links0, peak0, on), _, _ = _schedule(name, monkeypatch, cap=1 << 50, **kw)
        assert not on and peak0 == peak
        assert links0 == [None if l is None else l[:3] + ((0, 0),) for l in links]


def test_schedule_budgets_the_first_level_first(monkeypatch):
    name = "48 deep, shift 24"
    _, (links, peak, level1), pair, triple = _schedule(name, monkeypatch, cap=1 << 50, n_streams=3)
    assert level1 and peak == 2 + 3      # two sets alive along the chain, one spare per stream
    _, (links0, peak0, on), _, _ = _schedule(name, monkeypatch, cap=peak * (pair + triple) - 1, n_streams=3)
    assert (peak0, on) == (peak, False) and all(l is None or l[3] == (0, 0) for l in links0)
    assert [l and l[:3] for l in links0] == [l and l[:3] for l in links]
    _, got, _, _ = _schedule(name, monkeypatch, cap=peak * (pair + triple), n_streams=3)
    assert got == (links, peak, True)
    _, got, _, _ = _schedule(name, monkeypatch, cap=peak * pair - 1, n_streams=3)
    assert got == (None, 0, False)
    _, (_, _, on), _, _ = _schedule(name, monkeypatch, cap=1 << 50, free=2 * peak * (pair + triple) - 2, n_streams=3)
    assert not on
    # the bench: 17 sets on one stream, 20 on three, both inside the default cap
    for n_streams, sets in ((1, 17), (3, 20)):
        monkeypatch.undo()
        _, (links, peak, level1), pair, triple = _schedule("bench", monkeypatch, n_streams=n_streams)
        assert (peak, level1) == (sets, True) and peak * (pair + triple) <= inference.CARRY_POOL_BYTES


def test_a_batch_passes_on_only_planes_it_computes(monkeypatch):
    # z stride 16 under a depth of 48: a batch would take over planes [6, 30) and pass on its [22, 46). The tiles
    # of [22, 30) are not computed there, so nothing could store them again: the chain is cut at every second batch
    PLANS["cut"] = ((112, 32, 96), (48, 32, 64), (32, 8, 32), 2, None)
    try:
        succ, (links, peak, level1), _, _ = _schedule("cut", monkeypatch, cap=1 << 50)
    finally:
        del PLANS["cut"]
    assert succ == [1, 2, 3, 4, None]
    assert links == [(1, 16, (6, 30), (4, 12)), None, (3, 16, (6, 30), (4, 12)), None, None]
    assert (peak, level1) == (2, True)
    # where only the second level's ranges meet, only that level is cut (an engine made up for the purpose: the
    # first level takes [4, 12) and passes on [20, 28); the second would take [4, 16) and pass on [12, 24))

    class Odd(_Model):
        def carry_planes(self, shape, row_stride, shift_z, device=None):
            return (4, 12)

        def carry1_planes(self, shape, row_stride, shift_z, device=None):
            return (4, 16)

    shape, patch, overlap, batch_size = (112, 32, 96), (48, 32, 64), (32, 8, 32), 2
    starts = list(inference.generate_patch_starts((1, 1) + shape, patch, overlap))
    monkeypatch.setattr(inference, "CARRY_POOL_BYTES", 1 << 50)
    links, peak, level1 = inference._carry_schedule(Odd(), succ, starts, batch_size, patch, overlap, 1, None, free=1 << 50)
    assert level1 and [l[:3] for l in links[:4]] == [(i + 1, 16, (4, 12)) for i in range(4)] and links[4] is None
    assert [l[3] for l in links[:4]] == [(4, 16), (0, 0), (4, 16), (0, 0)]
