"""
The first level's carried planes with the border launch carrying too and inc.0 skipping the planes no launch reads
(engine.hip: kRowStagesCarry, conv_first_skip_planes), against EXASPIM_OPT_CARRY_MAIN_ONLY, which restores the
launches that carry in the main launch only.

Through the C ABI: A (carry out) then B (carry in) on one seeded volume, with B's workspace refilled after A -- the
planes inc.0 skips then hold the fill, NaN bits for 0xFF and 0x7F. B must equal B alone (the clipped entry) and B
under the option bit, bit for bit inside the kept box, with the second level's carry present and absent. predict()
on a device volume of two z slabs and two rows gives the same array with the option off and on, on one stream and
on three, with inference.CARRY_Z1 on and off. Geometries, fills and helpers are test_gpu_carry_forward.py's and
test_gpu_carry1_forward.py's.
"""

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from test_gpu_bf16x3 import dev, make_model  # noqa: F401  (fixture)
from test_gpu_carry1_forward import _buffers, _carry1, _forward
from test_gpu_carry_forward import (FILLS, GEOMETRIES, SENTINEL, SENTINEL_WORD, TRIM, _carry, _guarded, _intact,
                                    _setup, state)  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _a_then_b(S, dev, name, fill, level1):  # noqa: F811
    """B's kept output after A carried out into B's buffers and the workspace was refilled; every guarded buffer."""
    model = S["model"]
    patch, stride, shift, span = GEOMETRIES[name]
    d, h, w = patch
    bufs = _buffers(model, patch, fill, dev)
    t = [b[1] for b in bufs]
    a_pair, a_triple, b_pair, b_triple = t[:2], t[2:5], t[5:7], t[7:]
    ws_raw, ws = _guarded(S["need"], fill, dev)
    numel = 2 * 3 * d * h * w
    out_raw, out = _guarded(4 * numel, SENTINEL, dev)
    out_a = torch.empty(numel, dtype=torch.float32, device=dev)
    ca = _carry(a_pair, out=b_pair, out_z=(span[0] + shift, span[1] + shift), out_shift=shift)
    cb = _carry(b_pair, in_z=span)
    ca1 = cb1 = None
    if level1:
        span1 = model.carry1_planes((2,) + patch, stride, shift, dev)
        if span1[1] > span1[0]:
            ca1 = _carry1(a_triple, out=b_triple, out_z=(span1[0] + shift // 2, span1[1] + shift // 2),
                          out_shift=shift // 2)
            cb1 = _carry1(b_triple, in_z=span1)
        # (no level-1 range at this geometry, 32 x 16 x 64: the entry without the second level's buffers)
    assert _forward(S, dev, 0, out_a, ca, ca1, ws, patch, stride) == 0, _native.last_error()
    ws.fill_(fill)     # (B must not depend on what A left in the workspace; inc.0's skipped planes keep the fill)
    assert _forward(S, dev, 1, out, cb, cb1, ws, patch, stride) == 0, _native.last_error()
    got = out.view(torch.float32).view(2, 3, d, h, w).cpu()
    intact = all(_intact(raw, fill) for raw, _ in bufs) and _intact(ws_raw, fill) and _intact(out_raw, SENTINEL)
    return got, intact


@pytest.mark.parametrize("level1", [True, False], ids=["carry1", "carry"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_carried_forward_equals_the_forward_alone_and_the_main_only_carry(state, dev, dtype, name, level1):  # noqa: F811
    S = _setup(state, dev, dtype, name)
    patch, stride, shift, span = GEOMETRIES[name]
    assert S["model"].carry_planes((2,) + patch, stride, shift, dev) == span
    kept = torch.zeros((2, 3) + patch, dtype=torch.bool)
    kept[(Ellipsis,) + tuple(slice(TRIM, p - TRIM) for p in patch)] = True
    lib = _native.lib()
    try:
        _native.check(lib.exaspim_unet_set_options(S["handle"], _native.OPT_CARRY_MAIN_ONLY), "set_options")
        main_only, intact = _a_then_b(S, dev, name, FILLS[1], level1)
    finally:
        _native.check(lib.exaspim_unet_set_options(S["handle"], 0), "set_options")
    assert intact
    for fill in FILLS:
        got, intact = _a_then_b(S, dev, name, fill, level1)
        for want, what in ((S["want"], "B alone"), (main_only, "EXASPIM_OPT_CARRY_MAIN_ONLY")):
            differ = got.view(torch.int32)[kept] != want.view(torch.int32)[kept]
            assert not differ.any(), (f"fill {fill:#x} against {what}: {int(differ.sum())} of {int(kept.sum())} kept "
                                      f"voxels differ, first at {kept.nonzero()[differ][:4].tolist()}")
        assert not bool(torch.isnan(got[kept]).any())
        assert bool((got.view(torch.int32)[~kept] == SENTINEL_WORD).all()), "voxels outside the kept box were written"
        assert intact, f"fill {fill:#x}: a guard band"


def test_set_options_accepts_the_new_bit(state, dev):  # noqa: F811
    S = _setup(state, dev, "fp16", "32x16x64")
    lib = _native.lib()
    try:
        assert lib.exaspim_unet_set_options(S["handle"], _native.OPT_CARRY_MAIN_ONLY) == 0
        assert lib.exaspim_unet_set_options(S["handle"], _native.OPT_CARRY_MAIN_ONLY | _native.OPT_ROW_SEPARATE_BORDERS) == 0
        assert lib.exaspim_unet_set_options(S["handle"], 1024) == -1 and "unknown option" in _native.last_error()
    finally:
        _native.check(lib.exaspim_unet_set_options(S["handle"], 0), "set_options")


# two z slabs, two rows along y, two patches per row
PREDICT = ((48, 24, 96), dict(batch_size=2, patch_shape=(32, 16, 64), overlap=(16, 8, 32), trim=TRIM))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_predict_is_the_same_with_the_option_off_and_on(state, dev, dtype, monkeypatch):  # noqa: F811
    if ("model", dtype) not in state:
        state[("model", dtype)] = make_model(dev, compute_dtype=dtype)[0]
    model = state[("model", dtype)]
    shape, kw = PREDICT
    vol = inference.DeviceVolume.from_array(synthetic.synth_volume(shape, seed=59), dev)
    carried = []
    run_prepared = model.run_prepared

    def counting(*args, **kwargs):
        carried.append(kwargs.get("carry") is not None)
        return run_prepared(*args, **kwargs)

    monkeypatch.setattr(model, "run_prepared", counting)
    assert model.engine_options == 0 and inference.CARRY_Z
    want = None
    try:
        for options in (_native.OPT_CARRY_MAIN_ONLY, 0):
            model.engine_options = options
            for carry_z1 in (True, False):
                monkeypatch.setattr(inference, "CARRY_Z1", carry_z1)
                for n_streams in (1, 3):
                    del carried[:]
                    got = inference.predict(vol, model, verbose=False, n_streams=n_streams, **kw)
                    assert len(carried) == 4 and all(carried), carried      # two chains of two rows
                    if want is None:
                        want = got
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (options, carry_z1, n_streams)
    finally:
        model.engine_options = 0
    monkeypatch.setattr(inference, "CARRY_Z", False)
    del carried[:]
    got = inference.predict(vol, model, verbose=False, n_streams=1, **kw)
    assert carried and not any(carried)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "against the forward without carried planes"
