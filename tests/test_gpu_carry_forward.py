"""
exaspim_unet_forward_prepared_carry: the first level's skip tensor and its max-pool in caller buffers,
with planes carried from a forward A to the forward B that lies `shift` planes further down the volume.

Through the C ABI: A (carry out) then B (carry in) on one seeded volume, against B alone through
exaspim_unet_forward_prepared_clipped: the same bits on the kept voxels whatever B's buffers and the
workspace held before A ran, guards intact. Requests the engine cannot honour are refused before
anything is launched. predict() on a device volume with inference.CARRY_Z on gives the array it gives with it off, on one
stream and on three, and with a cap that forces the fall-back.
"""

import ctypes

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from test_gpu_bf16x3 import dev, make_model  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL, SENTINEL_WORD = 0x5A, 0x5A5A5A5A
TRIM = 4
# patch, row stride, z shift, the planes B takes over
GEOMETRIES = {"96x16x96": ((96, 16, 96), 64, 64, (6, 30)), "32x16x64": ((32, 16, 64), 32, 16, (4, 12))}
FILLS = [0x00, 0xFF, 0x7F]


@pytest.fixture(scope="module")
def state(dev):  # noqa: F811
    s = {}
    yield s
    s.clear()


def _setup(state, dev, dtype, name):  # noqa: F811
    """Model, prepared batches of A and B, and B's reference output through the clipped entry."""
    key = (dtype, name)
    if key in state:
        return state[key]
    if ("model", dtype) not in state:
        state[("model", dtype)] = make_model(dev, compute_dtype=dtype)[0]
    model = state[("model", dtype)]
    patch, stride, shift, _ = GEOMETRIES[name]
    d, h, w = patch
    vol = synthetic.synth_volume((d + shift, h, w + stride), seed=77)
    mn, mx = np.percentile(np.minimum(vol, 1000), (1, 99.9))
    dvol = inference.DeviceVolume.from_array(vol, dev)
    layout = model.input_layout(dev)
    prepared = []
    for z in (0, shift):
        starts = torch.tensor([(z, 0, 0), (z, 0, stride)], dtype=torch.int32, device=dev)
        prepared.append(inference._get_batch_inputs(dvol, starts, patch, dev, clip=np.uint16(1000), mn=mn, mx=mx,
                                                    layout=layout))
    lib = _native.lib()
    handle = model._ensure_engine(dev)
    need = lib.exaspim_unet_workspace_bytes(handle, 2, d, h, w)
    assert need, _native.last_error()
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    want = torch.empty((2, 3, d, h, w), dtype=torch.float32, device=dev)
    keep_hi = _native.int3((d - TRIM, h - TRIM, w - TRIM))
    _native.check(lib.exaspim_unet_forward_prepared_clipped(
        handle, prepared[1].data_ptr(), want.data_ptr(), 2, d, h, w, 1, TRIM, stride, keep_hi, ws.data_ptr(), need,
        torch.cuda.current_stream(dev).cuda_stream), "clipped")
    torch.cuda.synchronize()
    state[key] = dict(model=model, handle=handle, prepared=prepared, want=want.cpu(), need=need, keep_hi=keep_hi)
    return state[key]


def _guarded(nbytes, fill, dev):  # noqa: F811
    raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return raw, raw[GUARD:GUARD + nbytes]


def _intact(raw, fill):
    return bool((raw[:GUARD] == fill).all() and (raw[-GUARD:] == fill).all())


def _carry(own, in_z=(0, 0), out=None, out_z=(0, 0), out_shift=0):
    c = _native.UNetCarry()
    c.own_skip, c.own_pool = (t.data_ptr() if t is not None else None for t in own)
    c.in_z[:] = in_z
    if out is not None:
        c.out_skip, c.out_pool = (t.data_ptr() if t is not None else None for t in out)
    c.out_z[:] = out_z
    c.out_shift = out_shift
    return c


def _forward(S, dev, which, out, carry, ws, patch, stride):  # noqa: F811
    d, h, w = patch
    rc = _native.lib().exaspim_unet_forward_prepared_carry(
        S["handle"], S["prepared"][which].data_ptr(), out.data_ptr(), 2, d, h, w, 1, TRIM, stride, S["keep_hi"],
        ctypes.byref(carry), ws.data_ptr(), S["need"], torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_carried_forward_equals_the_forward_alone(state, dev, dtype, name):  # noqa: F811
    S = _setup(state, dev, dtype, name)
    model = S["model"]
    patch, stride, shift, span = GEOMETRIES[name]
    d, h, w = patch
    assert model.carry_planes((2,) + patch, stride, shift, dev) == span
    skip_elems, pool_elems = model.carry_pair_elems((2,) + patch)
    kept = torch.zeros((2, 3) + patch, dtype=torch.bool)
    kept[(Ellipsis,) + tuple(slice(TRIM, p - TRIM) for p in patch)] = True
    for fill in FILLS:
        bufs = [_guarded(2 * e, fill, dev) for e in (skip_elems, pool_elems, skip_elems, pool_elems)]
        (a_skip, a_pool), (b_skip, b_pool) = [b[1] for b in bufs[:2]], [b[1] for b in bufs[2:]]
        ws_raw, ws = _guarded(S["need"], fill, dev)
        numel = 2 * 3 * d * h * w
        out_raw, out = _guarded(4 * numel, SENTINEL, dev)
        out_a = torch.empty(numel, dtype=torch.float32, device=dev)
        ca = _carry((a_skip, a_pool), out=(b_skip, b_pool), out_z=(span[0] + shift, span[1] + shift), out_shift=shift)
        assert _forward(S, dev, 0, out_a, ca, ws, patch, stride) == 0, _native.last_error()
        ws.fill_(fill)     # (B must not depend on what A left in the workspace either)
        cb = _carry((b_skip, b_pool), in_z=span)
        assert _forward(S, dev, 1, out, cb, ws, patch, stride) == 0, _native.last_error()
        got = out.view(torch.float32).view(2, 3, d, h, w).cpu()
        differ = got.view(torch.int32)[kept] != S["want"].view(torch.int32)[kept]
        assert not differ.any(), (f"fill {fill:#x}: {int(differ.sum())} of {int(kept.sum())} kept voxels differ, "
                                  f"first at {kept.nonzero()[differ][:4].tolist()}")
        assert not bool(torch.isnan(got[kept]).any())
        assert bool((got.view(torch.int32)[~kept] == SENTINEL_WORD).all()), "voxels outside the kept box were written"
        for raw, _ in bufs:
            assert _intact(raw, fill), f"fill {fill:#x}: guard of a carry buffer"
        assert _intact(ws_raw, fill) and _intact(out_raw, SENTINEL)


BAD = ["odd in", "misaligned in", "in beyond d - 2", "out not the successor's range", "out without pool",
       "no own pool", "no row", "per-patch encoder"]


@pytest.mark.parametrize("what", BAD)
def test_requests_the_engine_cannot_honour_are_refused(state, dev, what):  # noqa: F811
    name = "32x16x64"
    S = _setup(state, dev, "fp16", name)
    patch, stride, shift, span = GEOMETRIES[name]
    d, h, w = patch
    skip_elems, pool_elems = S["model"].carry_pair_elems((2,) + patch)
    bufs = [_guarded(2 * e, SENTINEL, dev) for e in (skip_elems, pool_elems, skip_elems, pool_elems)]
    (a_skip, a_pool), (b_skip, b_pool) = [b[1] for b in bufs[:2]], [b[1] for b in bufs[2:]]
    good_out = dict(out=(b_skip, b_pool), out_z=(span[0] + shift, span[1] + shift), out_shift=shift)
    carry = {
        "odd in": _carry((a_skip, a_pool), in_z=(5, 12)),
        "misaligned in": _carry((a_skip, a_pool), in_z=(6, 12)),
        "in beyond d - 2": _carry((a_skip, a_pool), in_z=(24, 32)),
        "out not the successor's range": _carry((a_skip, a_pool), **dict(good_out, out_z=(22, 30))),
        "out without pool": _carry((a_skip, a_pool), **dict(good_out, out=(b_skip, None))),
        "no own pool": _carry((a_skip, None), in_z=span),
        "no row": _carry((a_skip, a_pool), in_z=span),
        "per-patch encoder": _carry((a_skip, a_pool), in_z=span),
    }[what]
    ws_raw, ws = _guarded(S["need"], SENTINEL, dev)
    out_raw, out = _guarded(4 * 2 * 3 * d * h * w, SENTINEL, dev)
    lib = _native.lib()
    try:
        if what == "per-patch encoder":
            _native.check(lib.exaspim_unet_set_options(S["handle"], _native.OPT_PER_PATCH_ENCODER), "set_options")
            span_now = (ctypes.c_int32 * 2)()
            _native.check(lib.exaspim_unet_carry_planes(S["handle"], 2, d, h, w, stride, shift, span_now), "planes")
            assert tuple(span_now) == (0, 0)
        rc = _forward(S, dev, 1, out, carry, ws, patch, 0 if what == "no row" else stride)
    finally:
        _native.check(lib.exaspim_unet_set_options(S["handle"], 0), "set_options")
    assert rc == -1, (rc, _native.last_error())      # EXASPIM_E_INVALID
    assert "carr" in _native.last_error(), _native.last_error()
    for raw, _ in bufs + [(ws_raw, ws), (out_raw, out)]:      # nothing was launched
        assert bool((raw == SENTINEL).all())


PREDICTS = {
    "224x16x160": ((224, 16, 160), dict(batch_size=2, patch_shape=(96, 16, 96), overlap=(32, 8, 32), trim=TRIM)),
    "64x16x96": ((64, 16, 96), dict(batch_size=2, patch_shape=(32, 16, 64), overlap=(16, 8, 32), trim=TRIM)),
}


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(PREDICTS))
def test_predict_is_the_same_with_and_without_carry(state, dev, dtype, name, monkeypatch):  # noqa: F811
    if ("model", dtype) not in state:
        state[("model", dtype)] = make_model(dev, compute_dtype=dtype)[0]
    model = state[("model", dtype)]
    shape, kw = PREDICTS[name]
    # (a device volume: predict() then runs the whole window in one run_sliding_window call; a host array goes
    # through the slab pipeline, whose calls do not carry from one to the next)
    vol = inference.DeviceVolume.from_array(synthetic.synth_volume(shape, seed=53), dev)
    carried = []
    run_prepared = model.run_prepared

    def counting(*args, **kwargs):
        carried.append(kwargs.get("carry") is not None)
        return run_prepared(*args, **kwargs)

    monkeypatch.setattr(model, "run_prepared", counting)
    monkeypatch.setattr(inference, "CARRY_Z", False)
    want = inference.predict(vol, model, verbose=False, n_streams=1, **kw)
    assert carried and not any(carried)
    monkeypatch.setattr(inference, "CARRY_Z", True)
    for n_streams in (1, 3):
        del carried[:]
        got = inference.predict(vol, model, verbose=False, n_streams=n_streams, **kw)
        assert len(carried) == 3 and all(carried), carried      # three rows of two patches, one chain
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{n_streams} stream(s)"
    monkeypatch.setattr(inference, "CARRY_POOL_BYTES", 1 << 10)     # no room for the buffers: every batch on its own
    del carried[:]
    got = inference.predict(vol, model, verbose=False, n_streams=3, **kw)
    assert len(carried) == 3 and not any(carried)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
