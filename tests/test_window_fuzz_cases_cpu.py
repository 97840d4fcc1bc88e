"""The case list of test_gpu_window_fuzz.py, planned on the host (carry_ref.py's model of the engine's plane
rule through inference.carry_plan and inference._carry_schedule): the committed seed must give cases that reach
what the GPU test is for -- links across several batches, second-level ranges, cut chains, carried batches that
are clipped as well, row and non-row batches in one call, and cases that carry nothing. On the GPU that test
asserts that the real engine's links are this model's for every case."""

import ctypes

import pytest

import layer_ref as R
import window_fuzz_cases as W
from aind_exaspim_neuron_segmentation_amd import _native, inference

CASES = W.cases(W.COMMITTED_CASES, W.COMMITTED_SEED)      # (whatever the environment asks the GPU test to run)


def test_cases_stay_small_and_inside_the_described_ranges():
    assert len(CASES) == W.COMMITTED_CASES + len(W.HAND)
    for c in CASES:
        t = W.traits(c)
        assert t["patches"] <= W.MAX_PATCHES and t["patches"] * c["patch"][0] * c["patch"][1] * c["patch"][2] <= \
            W.MAX_PATCH_VOXELS, c
        assert c["patch"][0] in (32, 48, 64) and c["patch"][1] in (16, 32) and c["patch"][2] in (64, 96), c
        assert c["overlap"][2] in (16, 32) and (c["patch"][0] - c["overlap"][0]) % 2 == 0 and c["trim"] in (0, 2, 4), c
        inference.SlidingWindow(c["shape"], c["patch"], c["overlap"], c["trim"])      # a geometry predict() accepts
    for c in W.generated(W.COMMITTED_CASES, W.COMMITTED_SEED):
        counts = [len(r) for r in inference._start_ranges(c["shape"], c["patch"], c["overlap"])]
        assert 2 <= counts[0] <= 4 and 1 <= counts[1] <= 3 and 2 <= counts[2] <= 4, (c, counts)


def test_the_committed_list_reaches_what_the_gpu_test_is_for():
    ts = [W.traits(c) for c in CASES]
    count = lambda key: sum(bool(t[key]) for t in ts)     # noqa: E731
    print({k: count(k) for k in ("links", "far", "level1", "cuts", "clipped_links", "mixed")},
          "nothing carried:", sum(t["links"] == 0 for t in ts), "of", len(ts))
    assert 2 * count("links") >= len(ts)          # a link at all
    assert count("far") >= 4                      # a successor more than one batch later
    assert count("level1") >= 4                   # a second-level range
    assert count("cuts") >= 2                     # a chain cut where a batch would pass on planes it takes over
    assert count("clipped_links") >= 3            # a link whose predecessor or successor is clipped to the volume
    assert count("mixed") >= 1                    # row and non-row batches in one call
    assert sum(t["links"] == 0 for t in ts) >= 2  # nothing carried at all


def test_hand_written_cases_plan_as_intended():
    t = [W.traits(c) for c in W.HAND]
    p = [W.plan(c) for c in W.HAND]
    # 12 batches, 9 links, the successor 3 batches later, all with a level-1 range, 3 links touch a clipped batch
    assert (t[0]["batches"], t[0]["links"], t[0]["distances"], t[0]["level1"], t[0]["clipped_links"]) == (12, 9, [3], 9, 3)
    # 16 batches, 8 of them rows, links 4 batches apart, row and non-row batches mixed
    assert (t[1]["batches"], t[1]["rows"], t[1]["distances"], t[1]["mixed"]) == (16, 8, [4], True) and t[1]["links"] > 0
    # the chain cut at every second batch
    assert (t[2]["links"], t[2]["cuts"]) == (4, 4)
    assert [l is not None for l in p[2]["links"]] == [True, True, False, False, True, True, False, False, False, False]
    # level 0 only, links 2 apart
    assert t[3]["links"] > 0 and t[3]["level1"] == 0 and t[3]["distances"] == [2] and not p[3]["level1"]
    # a batch spans two rows: nothing carries
    assert t[4]["links"] == 0 and t[4]["rows"] == 0 and set(p[4]["succ"]) == {None}
    # rows for carry_plan that the engine runs per patch: nothing carries either
    assert t[5]["links"] == 0 and t[5]["rows"] == 0 and any(s is not None for s in p[5]["succ"])
    # the six counts over the hand-written cases alone
    assert [sum(bool(x[k]) for x in t) for k in ("links", "far", "level1", "cuts", "clipped_links", "mixed")] == \
        [4, 4, 3, 1, 2, 1]


@pytest.fixture(scope="module")
def probe():
    import __graft_entry__

    __graft_entry__.build()
    lib = ctypes.CDLL(R.PROBE_PATH)
    i32 = ctypes.c_int32
    lib.probe_conv_carry_tile_depth.restype = i32
    lib.probe_conv_carry_tile_depth.argtypes = [i32, i32, i32, i32, i32, i32, i32, ctypes.c_size_t]
    lib.probe_conv_row_mode_ok.restype = i32
    lib.probe_conv_row_mode_ok.argtypes = [i32] * 6
    return lib


def test_the_host_model_is_the_launchers_answer_for_every_batch(probe):
    """carry_ref's row_mode is conv_row_mode_ok for inc.3 of the full-width network (32 couts), and its level-1
    tile depth of 4 is what the launcher reports for down1.0 and down1.3 at every batch shape that carries."""
    for c in CASES:
        d, h, w = c["patch"]
        p = W.plan(c)
        for b in p["batches"]:
            stride = inference.batch_row_stride(b, c["patch"], c["overlap"])
            for dt in (_native.DT_F16, _native.DT_BF16):
                assert probe.probe_conv_row_mode_ok(dt, 32, len(b), w, stride, 1) == int(W.row_mode(len(b), w, stride)), (c, b)
        for n in {len(p["batches"][bi]) for bi, l in enumerate(p["links"]) if l is not None and l[3][1] > l[3][0]}:
            scratch = (d + 2) * (h + 2) * (w + 2) * 4
            for dt in (_native.DT_F16, _native.DT_BF16):
                for ca in (32, 64):
                    assert probe.probe_conv_carry_tile_depth(dt, ca, 64, n, d // 2, h // 2, w // 2, scratch) == 4, (c, n, ca)
