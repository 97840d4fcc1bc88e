"""
Seeded fuzz of the 16-bit sliding window's execution plans on the GPU (-m gpu): the benchmarked mode -- fp16 or
bf16 storage, the full-width network -- with every plan switch turned on one after the other, each rung bit for
bit the plain plan's result: the prepared gather, the trimmed forward, CLIP_TO_VOLUME, row mode, CARRY_Z,
CARRY_Z1, several streams, a carry pool that admits the first level only, and the slab pipeline of a host array.

The plain plan is anchored to predict() of the fp32 engine on the same weights (itself held to the CPU oracle by
test_gpu_fuzz.py) within test_gpu_parity.PROB_TOL_16BIT. On the carrying rungs a ledger of every run_prepared
call checks which batches carry what, in which buffers: the links are inference._carry_schedule's for the real
model, which are the host model's (carry_ref.py; test_window_fuzz_cases_cpu.py holds the case list to the
geometries this needs), and no buffer set is handed to anybody else between the forward that fills it and the
forward that reads it. The cases are fixed by the seed (window_fuzz_cases.py); a failure prints its case.
"""

import numpy as np
import pytest

import window_fuzz_cases as W
from aind_exaspim_neuron_segmentation_amd import _native, inference
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from carry_ref import _RowModel
from test_gpu_bf16x3 import dev, make_model  # noqa: F401  (fixture)
from test_gpu_parity import PROB_TOL_16BIT

pytestmark = pytest.mark.gpu

PROB_TOL = dict(PROB_TOL_16BIT)
CASES = W.cases()


@pytest.fixture(scope="module")
def state(dev):  # noqa: F811
    s = {}
    yield s
    s.clear()


def _model(state, dev, dtype):  # noqa: F811
    if ("model", dtype) not in state:
        state[("model", dtype)] = make_model(dev, compute_dtype=dtype)[0]     # full width, 3 output channels
    return state[("model", dtype)]


def _volume(case):
    return synthetic.synth_volume(case["shape"], seed=case["seed"])


def _kw(case):
    return dict(batch_size=case["batch"], patch_shape=case["patch"], overlap=case["overlap"], trim=case["trim"],
                verbose=False)


def _fp32_reference(state, dev, case):  # noqa: F811
    """predict() of the fp32 engine, once per case for both storage types."""
    key = ("fp32", W.case_id(case))
    if key not in state:
        vol = inference.DeviceVolume.from_array(_volume(case), dev)
        state[key] = inference.predict(vol, _model(state, dev, "fp32"), n_streams=1, **_kw(case))
    return state[key]


def _ptrs(buffers):
    return None if buffers is None else tuple(int(t.data_ptr()) for t in buffers)


def _ledger(model, monkeypatch):
    """Wraps model.run_prepared: one entry per call, in call order, which is batch order."""
    calls = []
    run_prepared = model.run_prepared

    def logging(*args, **kwargs):
        c = kwargs.get("carry")
        entry = None
        if c is not None:
            entry = dict(own=_ptrs(c["own"]), own1=_ptrs(c.get("own1")), out=_ptrs(c.get("out")),
                         out1=_ptrs(c.get("out1")), in_z=tuple(c.get("in_z", (0, 0))),
                         in_z1=tuple(c.get("in_z1", (0, 0))), out_z=c.get("out_z"), out_z1=c.get("out_z1"),
                         out_shift=c.get("out_shift"), out_shift1=c.get("out_shift1"))
        calls.append(entry)
        return run_prepared(*args, **kwargs)

    monkeypatch.setattr(model, "run_prepared", logging)
    return calls


def _check_ledger(calls, case, model, dev, n_streams, rung, level1_expected, host=_RowModel):  # noqa: F811
    """The carry dicts run_sliding_window handed out against the schedule of the real model, and that against the
    host model's (host(level1=...): carry_ref's stand-in for this network, by default the full-width one)."""
    p = W.plan(case, host(level1=level1_expected), n_streams)
    starts, batch, patch, overlap = p["starts"], case["batch"], case["patch"], case["overlap"]
    links, peak, level1 = inference._carry_schedule(model, p["succ"], starts, batch, patch, overlap, n_streams, dev)
    links = links or [None] * len(p["batches"])
    where = f"{rung}: {case}"
    assert len(calls) == len(p["batches"]), where
    if level1_expected:
        assert links == p["links"] and peak == p["peak"] and level1 == p["level1"], \
            f"{where}: the engine's links {links} are not the host model's {p['links']}"
    else:     # the same links with no second-level range
        assert [l and l[:3] for l in links] == [l and l[:3] for l in p["links"]] and peak == p["peak"], where
        assert not level1 and all(l is None or l[3] == (0, 0) for l in links), where
    pred = {l[0]: bi for bi, l in enumerate(links) if l is not None}
    sets = set()
    for bi, (call, link) in enumerate(zip(calls, links)):
        at = f"{where}, batch {bi}"
        if link is None and bi not in pred:
            assert call is None, f"{at}: a carry for a batch without a link"
            continue
        assert call is not None, f"{at}: no carry"
        sets.add(call["own"])
        assert (call["own1"] is not None) == level1, at
        if link is None:
            assert call["out"] is None and call["out1"] is None, f"{at}: carries out without a link"
        else:
            bj, shift, span, span1 = link
            assert shift == int(p["batches"][bj][0][0]) - int(p["batches"][bi][0][0]), at
            assert call["out"] is not None and call["out"] != call["own"], f"{at}: own and out are one set"
            sets.add(call["out"])
            assert tuple(call["out_z"]) == (span[0] + shift, span[1] + shift) and call["out_shift"] == shift, at
            if span1[1] > span1[0]:
                assert call["out1"] is not None and call["out1"] != call["own1"], at
                assert tuple(call["out_z1"]) == (span1[0] + shift // 2, span1[1] + shift // 2), at
                assert call["out_shift1"] == shift // 2, at
            else:
                assert call["out1"] is None, f"{at}: second-level planes carried out without a range"
            # the successor works in the set this batch filled, on the planes it filled, and nobody else got
            # that set in between
            after = calls[bj]
            assert after is not None and after["own"] == call["out"], f"{at}: batch {bj} does not own what {bi} filled"
            assert after["in_z"] == (call["out_z"][0] - shift, call["out_z"][1] - shift) == tuple(span), at
            if span1[1] > span1[0]:
                assert after["own1"] == call["out1"], at
                assert after["in_z1"] == (call["out_z1"][0] - shift // 2, call["out_z1"][1] - shift // 2) == tuple(span1), at
            else:
                assert after["in_z1"] == (0, 0), at
            for bk in range(bi + 1, bj):
                other = calls[bk]
                assert other is None or (other["own"] != call["out"] and other["out"] != call["out"]), \
                    f"{at}: batch {bk} was handed the set that waits for batch {bj}"
        if bi not in pred:
            assert call["in_z"] == (0, 0) and call["in_z1"] == (0, 0), f"{at}: planes carried in from nowhere"
    assert len(sets) <= peak, f"{where}: {len(sets)} buffer sets, the schedule allows {peak}"
    return links, peak, level1


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=W.case_id)
def test_every_plan_switch_keeps_the_bits_of_the_plain_plan(state, dev, dtype, case, monkeypatch):  # noqa: F811
    print(case)
    reference = _fp32_reference(state, dev, case)      # (before any switch is flipped)
    _ladder(_model(state, dev, dtype), reference, case, dtype, dev, monkeypatch)


def _ladder(model, reference, case, dtype, dev, monkeypatch, host_model=_RowModel, affinity_mode=True):  # noqa: F811
    """Every plan switch turned on one after the other on `model`, each rung against the plain plan; rung 0 against
    `reference`, the fp32 engine's predict(). host_model: _check_ledger's."""
    host = _volume(case)
    vol = inference.DeviceVolume.from_array(host, dev)     # one run_sliding_window call sees the whole window
    kw = dict(_kw(case), affinity_mode=affinity_mode)
    streams = 2 + case["seed"] % 2
    out_shape = ((3,) if affinity_mode else ()) + tuple(case["shape"])

    def switches(**values):
        for name, value in values.items():
            monkeypatch.setattr(inference, name, value)

    def same(got, rung):
        differ = got.view(np.uint32) != plain.view(np.uint32)
        assert not differ.any(), (f"rung {rung} differs from the plain plan in {int(differ.sum())} of {differ.size} "
                                  f"voxels, first at {np.argwhere(differ)[0].tolist()}, max |diff| "
                                  f"{float(np.abs(got - plain).max()):.3e}: {dtype} {case}")

    # rung 0: the plain plan
    switches(PLAIN_GATHER=True, FULL_PATCHES=True, CLIP_TO_VOLUME=False, CARRY_Z=False)
    monkeypatch.setattr(model, "engine_options", _native.OPT_PER_PATCH_ENCODER)
    plain = inference.predict(vol, model, n_streams=1, **kw)
    assert plain.shape == out_shape == reference.shape and plain.dtype == np.float32 and np.isfinite(plain).all()
    err = float(np.abs(plain - reference).max())
    print(f"plain {dtype} plan vs the fp32 engine: max |diff| = {err:.3e} (bound {PROB_TOL[dtype]:.0e})")
    assert err < PROB_TOL[dtype], f"rung 0 (plain plan) vs the fp32 engine: {err:.3e}: {dtype} {case}"

    switches(PLAIN_GATHER=False)
    same(inference.predict(vol, model, n_streams=1, **kw), "1 (prepared gather)")
    switches(FULL_PATCHES=False)
    same(inference.predict(vol, model, n_streams=1, **kw), "2 (trimmed forward)")
    switches(CLIP_TO_VOLUME=True)
    same(inference.predict(vol, model, n_streams=1, **kw), "3 (CLIP_TO_VOLUME)")
    monkeypatch.setattr(model, "engine_options", 0)
    same(inference.predict(vol, model, n_streams=1, **kw), "4 (row mode)")

    calls = _ledger(model, monkeypatch)
    switches(CARRY_Z=True, CARRY_Z1=False)
    same(inference.predict(vol, model, n_streams=1, **kw), "5 (CARRY_Z)")
    _check_ledger(calls, case, model, dev, 1, "rung 5 (CARRY_Z)", False, host_model)
    ledgers = {5: list(calls)}      # rung -> its run_prepared calls, for the caller
    switches(CARRY_Z1=True)
    del calls[:]
    same(inference.predict(vol, model, n_streams=1, **kw), "6 (CARRY_Z1)")
    _check_ledger(calls, case, model, dev, 1, "rung 6 (CARRY_Z1)", True, host_model)
    ledgers[6] = list(calls)
    del calls[:]
    same(inference.predict(vol, model, n_streams=streams, **kw), f"7 ({streams} streams)")
    n_batches = -(-len(W.plan(case)["starts"]) // case["batch"])
    links, peak, level1 = _check_ledger(calls, case, model, dev, min(streams, n_batches), f"rung 7 ({streams} streams)",
                                        True, host_model)
    ledgers[7] = list(calls)
    if level1:      # a pool that admits the first level's buffers and not the second's
        pair_bytes = 2 * sum(model.carry_pair_elems((case["batch"],) + tuple(case["patch"])))
        switches(CARRY_POOL_BYTES=peak * pair_bytes + 1)
        del calls[:]
        same(inference.predict(vol, model, n_streams=streams, **kw), "8 (first level only under the cap)")
        _check_ledger(calls, case, model, dev, min(streams, n_batches), "rung 8 (first level only under the cap)", False,
                      host_model)
        ledgers[8] = list(calls)
    monkeypatch.undo()      # every switch on, run_prepared and the engine options as they were
    assert model.engine_options == 0 and inference.CARRY_Z and inference.CARRY_Z1 and not inference.PLAIN_GATHER
    same(inference.predict(host, model, **kw), "9 (host array, slab pipeline)")
    return plain, ledgers
