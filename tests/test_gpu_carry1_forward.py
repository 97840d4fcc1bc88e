"""
exaspim_unet_forward_prepared_carry1: next to the first level's buffers, down1.0's output, the second level's
skip tensor and its max-pool in caller buffers, with planes of both levels carried from a forward A to the
forward B that lies `shift` planes further down the volume.

Through the C ABI: A (carry out) then B (carry in) on one seeded volume, against B alone through
exaspim_unet_forward_prepared_clipped: the same bits on the kept voxels whatever the caller's buffers and the
workspace held before, guards intact. Requests the engine cannot honour are refused before anything is
launched. predict() on a device volume gives the same array with inference.CARRY_Z1 on and off, on one stream
and on three, and under a cap that admits the first level's buffers only.
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
# patch, row stride, z shift, the level-1 planes B takes over
GEOMETRIES = {
    "48x16x64 shift 16": ((48, 16, 64), 32, 16, (4, 12)),
    "48x16x64 shift 24": ((48, 16, 64), 32, 24, (4, 8)),
    "64x32x96 shift 32": ((64, 32, 96), 64, 32, (4, 12)),
}
EMPTY = ((32, 16, 64), 32, 16)      # d/2 - shift/2 - 3 = 5: no whole tile from plane 4 on
FILLS = [0x00, 0xFF, 0x7F]


@pytest.fixture(scope="module")
def state(dev):  # noqa: F811
    s = {}
    yield s
    s.clear()


def _model(state, dev, dtype):  # noqa: F811
    if ("model", dtype) not in state:
        state[("model", dtype)] = make_model(dev, compute_dtype=dtype)[0]
    return state[("model", dtype)]


def _setup(state, dev, dtype, name, model=None, tag=None, keep_hi=None, sigmoid=1):  # noqa: F811
    """Model, prepared batches of A and B, and B's reference output through the clipped entry. model (with a tag
    for the cache): another network than this file's; keep_hi: a clip (default: none); sigmoid: 0 for logits."""
    key = (dtype, name) if model is None else (dtype, name, tag, keep_hi, sigmoid)
    if key in state:
        return state[key]
    model = _model(state, dev, dtype) if model is None else model
    patch, stride, shift, _ = GEOMETRIES[name]
    d, h, w = patch
    vol = synthetic.synth_volume((d + shift, h, w + stride), seed=79)
    mn, mx = np.percentile(np.minimum(vol, 1000), (1, 99.9))
    dvol = inference.DeviceVolume.from_array(vol, dev)
    layout = model.input_layout(dev)
    prepared, gather = [], []
    for z in (0, shift):
        starts = torch.tensor([(z, 0, 0), (z, 0, stride)], dtype=torch.int32, device=dev)
        prepared.append(inference._get_batch_inputs(dvol, starts, patch, dev, clip=np.uint16(1000), mn=mn, mx=mx,
                                                    layout=layout))
        gather.append((dvol, starts, patch, dev, dict(clip=np.uint16(1000), mn=mn, mx=mx)))
    lib = _native.lib()
    handle = model._ensure_engine(dev)
    need = lib.exaspim_unet_workspace_bytes(handle, 2, d, h, w)
    assert need, _native.last_error()
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    want = torch.empty((2, model.output_channels, d, h, w), dtype=torch.float32, device=dev)
    want.view(torch.uint8).fill_(SENTINEL)
    keep_hi = _native.int3(keep_hi or (d - TRIM, h - TRIM, w - TRIM))
    _native.check(lib.exaspim_unet_forward_prepared_clipped(
        handle, prepared[1].data_ptr(), want.data_ptr(), 2, d, h, w, sigmoid, TRIM, stride, keep_hi, ws.data_ptr(),
        need, torch.cuda.current_stream(dev).cuda_stream), "clipped")
    torch.cuda.synchronize()
    # (gather: the arguments of inference._get_batch_inputs for the float32 patches of A and B)
    state[key] = dict(model=model, handle=handle, prepared=prepared, want=want.cpu(), need=need, keep_hi=keep_hi,
                      gather=gather, sigmoid=sigmoid)
    return state[key]


def _guarded(nbytes, fill, dev):  # noqa: F811
    raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return raw, raw[GUARD:GUARD + nbytes]


def _intact(raw, fill):
    return bool((raw[:GUARD] == fill).all() and (raw[-GUARD:] == fill).all())


def _ptrs(ts):
    return (t.data_ptr() if t is not None else None for t in ts)


def _carry(own, in_z=(0, 0), out=None, out_z=(0, 0), out_shift=0):
    c = _native.UNetCarry()
    c.own_skip, c.own_pool = _ptrs(own)
    c.in_z[:] = in_z
    if out is not None:
        c.out_skip, c.out_pool = _ptrs(out)
    c.out_z[:] = out_z
    c.out_shift = out_shift
    return c


def _carry1(own, in_z=(0, 0), out=None, out_z=(0, 0), out_shift=0, reserved=0):
    c = _native.UNetCarry1()
    c.own_mid1, c.own_skip1, c.own_pool2 = _ptrs(own)
    c.in_z[:] = in_z
    if out is not None:
        c.out_mid1, c.out_skip1, c.out_pool2 = _ptrs(out)
    c.out_z[:] = out_z
    c.out_shift = out_shift
    c.reserved = reserved
    return c


def _forward(S, dev, which, out, carry, carry1, ws, patch, stride):  # noqa: F811
    d, h, w = patch
    rc = _native.lib().exaspim_unet_forward_prepared_carry1(
        S["handle"], S["prepared"][which].data_ptr(), out.data_ptr(), 2, d, h, w, S.get("sigmoid", 1), TRIM, stride,
        S["keep_hi"],
        ctypes.byref(carry) if carry is not None else None, ctypes.byref(carry1) if carry1 is not None else None,
        ws.data_ptr(), S["need"], torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc


def _buffers(model, patch, fill, dev):  # noqa: F811
    """Guarded buffers of A's and B's pair and triple: [(raw, tensor)] * 10."""
    pair, triple = model.carry_pair_elems((2,) + patch), model.carry_triple_elems((2,) + patch)
    return [_guarded(2 * e, fill, dev) for e in pair + triple + pair + triple]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_carried_forward_equals_the_forward_alone(state, dev, dtype, name):  # noqa: F811
    S = _setup(state, dev, dtype, name)
    model = S["model"]
    patch, stride, shift, span1 = GEOMETRIES[name]
    d, h, w = patch
    span = model.carry_planes((2,) + patch, stride, shift, dev)
    assert span[1] > span[0]
    assert model.carry1_planes((2,) + patch, stride, shift, dev) == span1
    kept = torch.zeros((2, 3) + patch, dtype=torch.bool)
    kept[(Ellipsis,) + tuple(slice(TRIM, p - TRIM) for p in patch)] = True
    for fill in FILLS:
        bufs = _buffers(model, patch, fill, dev)
        t = [b[1] for b in bufs]
        a_pair, a_triple, b_pair, b_triple = t[:2], t[2:5], t[5:7], t[7:]
        ws_raw, ws = _guarded(S["need"], fill, dev)
        numel = 2 * 3 * d * h * w
        out_raw, out = _guarded(4 * numel, SENTINEL, dev)
        out_a = torch.empty(numel, dtype=torch.float32, device=dev)
        ca = _carry(a_pair, out=b_pair, out_z=(span[0] + shift, span[1] + shift), out_shift=shift)
        ca1 = _carry1(a_triple, out=b_triple, out_z=(span1[0] + shift // 2, span1[1] + shift // 2), out_shift=shift // 2)
        assert _forward(S, dev, 0, out_a, ca, ca1, ws, patch, stride) == 0, _native.last_error()
        ws.fill_(fill)     # (B must not depend on what A left in the workspace either)
        cb, cb1 = _carry(b_pair, in_z=span), _carry1(b_triple, in_z=span1)
        assert _forward(S, dev, 1, out, cb, cb1, ws, patch, stride) == 0, _native.last_error()
        got = out.view(torch.float32).view(2, 3, d, h, w).cpu()
        differ = got.view(torch.int32)[kept] != S["want"].view(torch.int32)[kept]
        assert not differ.any(), (f"fill {fill:#x}: {int(differ.sum())} of {int(kept.sum())} kept voxels differ, "
                                  f"first at {kept.nonzero()[differ][:4].tolist()}")
        assert not bool(torch.isnan(got[kept]).any())
        assert bool((got.view(torch.int32)[~kept] == SENTINEL_WORD).all()), "voxels outside the kept box were written"
        for raw, _ in bufs:
            assert _intact(raw, fill), f"fill {fill:#x}: guard of a carry buffer"
        assert _intact(ws_raw, fill) and _intact(out_raw, SENTINEL)


def test_own_buffers_without_any_carried_plane(state, dev):  # noqa: F811
    # the triple in use with nothing carried in or out: the forward alone
    name = "48x16x64 shift 16"
    S = _setup(state, dev, "fp16", name)
    patch, stride, shift, _ = GEOMETRIES[name]
    d, h, w = patch
    t = [b[1] for b in _buffers(S["model"], patch, 0xFF, dev)]
    ws = torch.full((S["need"],), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.empty(2 * 3 * d * h * w, dtype=torch.float32, device=dev)
    assert _forward(S, dev, 1, out, _carry(t[:2]), _carry1(t[2:5]), ws, patch, stride) == 0, _native.last_error()
    kept = torch.zeros((2, 3) + patch, dtype=torch.bool)
    kept[(Ellipsis,) + tuple(slice(TRIM, p - TRIM) for p in patch)] = True
    got = out.view(2, 3, d, h, w).cpu()
    assert torch.equal(got.view(torch.int32)[kept], S["want"].view(torch.int32)[kept])


def test_empty_range(state, dev):  # noqa: F811
    model = _model(state, dev, "fp16")
    patch, stride, shift = EMPTY
    span = model.carry_planes((2,) + patch, stride, shift, dev)
    assert span[1] > span[0], "the first level carries at this geometry"
    assert model.carry1_planes((2,) + patch, stride, shift, dev) == (0, 0)
    # ... and wherever the first level has nothing to carry, an odd shift, a level-1 shift that is odd
    assert model.carry1_planes((2, 48, 16, 64), 0, 16, dev) == (0, 0)      # no row
    assert model.carry1_planes((2, 48, 16, 64), 32, 15, dev) == (0, 0)
    assert model.carry1_planes((2, 48, 16, 64), 32, 18, dev) == (0, 0)
    assert model.carry1_planes((2, 48, 16, 64), 32, 16, dev) == (4, 12)
    f32 = _model(state, dev, "fp32")
    assert f32.carry1_planes((2, 48, 16, 64), 32, 16, dev) == (0, 0)


BAD = ["no first-level carry", "in without a first-level in", "misaligned in", "in below 3", "in beyond d/2 - 3",
       "out not the successor's range", "out without the first level's", "first level out by another shift",
       "out without pool", "no own mid", "reserved", "separate pools", "out of planes carried in"]


@pytest.mark.parametrize("what", BAD)
def test_requests_the_engine_cannot_honour_are_refused(state, dev, what):  # noqa: F811
    name = "48x16x64 shift 16"
    S = _setup(state, dev, "fp16", name)
    patch, stride, shift, span1 = GEOMETRIES[name]
    d, h, w = patch
    model = S["model"]
    span = model.carry_planes((2,) + patch, stride, shift, dev)
    bufs = _buffers(model, patch, SENTINEL, dev)
    t = [b[1] for b in bufs]
    a_pair, a_triple, b_pair, b_triple = t[:2], t[2:5], t[5:7], t[7:]
    s1 = shift // 2
    good0_out = dict(out=b_pair, out_z=(span[0] + shift, span[1] + shift), out_shift=shift)
    good1_out = dict(out=b_triple, out_z=(span1[0] + s1, span1[1] + s1), out_shift=s1)
    in0, out0 = _carry(a_pair, in_z=span), _carry(a_pair, **good0_out)
    carry, carry1 = {
        "no first-level carry": (None, _carry1(a_triple)),
        "in without a first-level in": (_carry(a_pair), _carry1(a_triple, in_z=span1)),
        "misaligned in": (in0, _carry1(a_triple, in_z=(6, 12))),
        "in below 3": (in0, _carry1(a_triple, in_z=(0, 8))),
        "in beyond d/2 - 3": (in0, _carry1(a_triple, in_z=(16, 24))),
        "out not the successor's range": (out0, _carry1(a_triple, **dict(good1_out, out_z=(12, 16)))),
        "out without the first level's": (in0, _carry1(a_triple, **good1_out)),
        "first level out by another shift": (
            _carry(a_pair, out=b_pair, out_z=(span[0] + 24, 18 + 24), out_shift=24), _carry1(a_triple, **good1_out)),
        "out without pool": (out0, _carry1(a_triple, **dict(good1_out, out=b_triple[:2] + [None]))),
        "no own mid": (in0, _carry1([None] + a_triple[1:], in_z=span1)),
        "reserved": (in0, _carry1(a_triple, in_z=span1, reserved=1)),
        "separate pools": (in0, _carry1(a_triple, in_z=span1)),
        # z shift 16 under a depth of 48: [22, 30) would be passed on, but is taken over and not computed here
        "out of planes carried in": (_carry(a_pair, in_z=span, **good0_out), None),
    }[what]
    ws_raw, ws = _guarded(S["need"], SENTINEL, dev)
    out_raw, out = _guarded(4 * 2 * 3 * d * h * w, SENTINEL, dev)
    lib = _native.lib()
    try:
        if what == "separate pools":
            _native.check(lib.exaspim_unet_set_options(S["handle"], _native.OPT_SEPARATE_DEEP_POOLS), "set_options")
            assert model.carry1_planes((2,) + patch, stride, shift, dev) == (0, 0)
        if what == "no first-level carry":
            # (the entry wants the first level's struct; the layers behind it refuse a triple without it as well)
            rc = lib.exaspim_unet_forward_prepared_carry1(
                S["handle"], S["prepared"][1].data_ptr(), out.data_ptr(), 2, d, h, w, 1, TRIM, stride, S["keep_hi"],
                None, ctypes.byref(carry1), ws.data_ptr(), S["need"], torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
        else:
            rc = _forward(S, dev, 1, out, carry, carry1, ws, patch, stride)
    finally:
        _native.check(lib.exaspim_unet_set_options(S["handle"], 0), "set_options")
    assert rc == -1, (rc, _native.last_error())      # EXASPIM_E_INVALID
    for raw, _ in bufs + [(ws_raw, ws), (out_raw, out)]:      # nothing was launched
        assert bool((raw == SENTINEL).all())


# volume, predict() arguments, and per batch of the one chain down z: carried at all, second level in, second level out
PREDICTS = {
    # z stride 24: every batch takes planes over and passes planes on
    "120x32x96 stride 24": ((120, 32, 96), dict(batch_size=2, patch_shape=(48, 32, 64), overlap=(24, 8, 32), trim=TRIM),
                            [1, 1, 1, 1], [0, 1, 1, 1], [1, 1, 1, 0]),
    # z stride 16: a batch would have to pass on planes [22, 30), which it takes over itself and does not compute;
    # the chain is cut at every second batch (and the last one has nobody to carry with)
    "112x32x96 stride 16": ((112, 32, 96), dict(batch_size=2, patch_shape=(48, 32, 64), overlap=(32, 8, 32), trim=TRIM),
                            [1, 1, 1, 1, 0], [0, 1, 0, 1, 0], [1, 0, 1, 0, 0]),
}


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(PREDICTS))
def test_predict_is_the_same_with_and_without_carry(state, dev, dtype, name, monkeypatch):  # noqa: F811
    model = _model(state, dev, dtype)
    shape, kw, any_carry, in1, out1 = PREDICTS[name]
    any_carry, in1, out1 = ([bool(v) for v in x] for x in (any_carry, in1, out1))
    # (a device volume: predict() then runs the whole window in one run_sliding_window call)
    vol = inference.DeviceVolume.from_array(synthetic.synth_volume(shape, seed=59), dev)
    seen = []     # per forward: (first level carried, second level carried in, second level carried out)
    run_prepared = model.run_prepared

    def counting(*args, **kwargs):
        c = kwargs.get("carry")
        seen.append((c is not None, bool(c and c.get("own1") is not None and c["in_z1"][1] > c["in_z1"][0]),
                     bool(c and c.get("out1") is not None)))
        return run_prepared(*args, **kwargs)

    monkeypatch.setattr(model, "run_prepared", counting)
    monkeypatch.setattr(inference, "CARRY_Z", False)
    want = inference.predict(vol, model, verbose=False, n_streams=1, **kw)
    n = len(seen)
    assert n == len(any_carry) and not any(any(s) for s in seen)      # z slabs of one row of two patches
    monkeypatch.setattr(inference, "CARRY_Z", True)
    monkeypatch.setattr(inference, "CARRY_Z1", False)
    del seen[:]
    got = inference.predict(vol, model, verbose=False, n_streams=1, **kw)
    assert [s[0] for s in seen] == any_carry and not any(s[1] or s[2] for s in seen)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "first level only"
    monkeypatch.setattr(inference, "CARRY_Z1", True)
    for n_streams in (1, 3):
        del seen[:]
        got = inference.predict(vol, model, verbose=False, n_streams=n_streams, **kw)
        assert [s[0] for s in seen] == any_carry
        assert [s[1] for s in seen] == in1 and [s[2] for s in seen] == out1, seen
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{n_streams} stream(s)"
    # a cap that admits the first level's buffers and not the second's
    starts = list(inference.generate_patch_starts((1, 1) + shape, kw["patch_shape"], kw["overlap"]))
    succ = inference.carry_plan(starts, 2, kw["patch_shape"], kw["overlap"])
    _, peak, level1 = inference._carry_schedule(model, succ, starts, 2, kw["patch_shape"], kw["overlap"], 3, dev)
    assert level1
    pair_bytes = 2 * sum(model.carry_pair_elems((2,) + kw["patch_shape"]))
    monkeypatch.setattr(inference, "CARRY_POOL_BYTES", peak * pair_bytes + 1)
    del seen[:]
    got = inference.predict(vol, model, verbose=False, n_streams=3, **kw)
    assert [s[0] for s in seen] == any_carry and not any(s[1] or s[2] for s in seen)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "first level only under the cap"
