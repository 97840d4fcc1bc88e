"""
exaspim_unet_forward_prepared_carry_y and predict() with rows carried along y.

Through the C ABI: the four batches (k, j), (k, j + 1), (k + 1, j), (k + 1, j + 1) of a 2 x 2 x 2 window of 64^3
patches run in plan order, each in caller buffers filled with the workspace fill (NaN bits for 0xFF and 0x7F), each
storing what the rule names into its successors' buffers -- the diagonal block among them, which only (k, j) can
give (k + 1, j + 1). Every batch must equal the same batch alone (the clipped entry) and the same chain under
EXASPIM_OPT_CARRY_NO_ROWS, bit for bit inside the kept box, with and without the second level's carry.
predict() on a device volume with ragged high faces gives the same array with inference.ROWS_CARRY_Y on and off, on one
stream and on three, under a pool that admits the z links' sets only, and on a cut y chain.
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
FILLS = [0x00, 0xFF, 0x7F]
PATCH, STRIDE, SHIFT = (64, 64, 64), 32, 32
ZC, YC = (4, 28), (8, 24)       # what a batch takes over: 4-plane tiles inside [2, 30), 8-row tiles inside [2, 30)
ORDER = [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.fixture(scope="module")
def state(dev):  # noqa: F811
    s = {}
    yield s
    s.clear()


def _guarded(nbytes, fill, dev):  # noqa: F811
    raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return raw, raw[GUARD:GUARD + nbytes]


def _intact(raw, fill):
    return bool((raw[:GUARD] == fill).all() and (raw[-GUARD:] == fill).all())


def _setup(state, dev, dtype):  # noqa: F811
    """Model, the prepared batches of the four (k, j) and each one's output alone through the clipped entry."""
    if dtype in state:
        return state[dtype]
    model = make_model(dev, compute_dtype=dtype)[0]
    d, h, w = PATCH
    vol = synthetic.synth_volume((d + SHIFT, h + SHIFT, w + STRIDE), seed=83)
    mn, mx = np.percentile(np.minimum(vol, 1000), (1, 99.9))
    dvol = inference.DeviceVolume.from_array(vol, dev)
    layout = model.input_layout(dev)
    lib = _native.lib()
    handle = model._ensure_engine(dev)
    need = lib.exaspim_unet_workspace_bytes(handle, 2, d, h, w)
    assert need, _native.last_error()
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    keep_hi = _native.int3((d - TRIM, h - TRIM, w - TRIM))
    prepared, want = {}, {}
    for k, j in ORDER:
        starts = torch.tensor([(k * SHIFT, j * SHIFT, 0), (k * SHIFT, j * SHIFT, STRIDE)], dtype=torch.int32, device=dev)
        prepared[k, j] = inference._get_batch_inputs(dvol, starts, PATCH, dev, clip=np.uint16(1000), mn=mn, mx=mx,
                                                     layout=layout)
        out = torch.empty((2, 3, d, h, w), dtype=torch.float32, device=dev)
        _native.check(lib.exaspim_unet_forward_prepared_clipped(
            handle, prepared[k, j].data_ptr(), out.data_ptr(), 2, d, h, w, 1, TRIM, STRIDE, keep_hi, ws.data_ptr(), need,
            torch.cuda.current_stream(dev).cuda_stream), "clipped")
        torch.cuda.synchronize()
        want[k, j] = out.cpu()
    state[dtype] = dict(model=model, handle=handle, prepared=prepared, want=want, need=need, keep_hi=keep_hi)
    return state[dtype]


def _structs(S, dev, sets, k, j, level1, event=None):  # noqa: F811
    """The three structs of batch (k, j): sets[(k, j)] = (pair, triple) of device tensors."""
    model = S["model"]
    c = _native.UNetCarry()
    c.own_skip, c.own_pool = (t.data_ptr() for t in sets[k, j][0])
    y = _native.UNetCarryY()
    c1 = None
    span1 = model.carry1_planes((2,) + PATCH, STRIDE, SHIFT, dev) if level1 else (0, 0)
    if level1:
        assert span1 == (4, 12)
        c1 = _native.UNetCarry1()
        c1.own_mid1, c1.own_skip1, c1.own_pool2 = (t.data_ptr() for t in sets[k, j][1])
    if k == 1:
        c.in_z[:] = ZC
        if level1:
            c1.in_z[:] = span1
    else:
        c.out_skip, c.out_pool = (t.data_ptr() for t in sets[1, j][0])
        c.out_z[:] = (ZC[0] + SHIFT, ZC[1] + SHIFT)
        c.out_shift = SHIFT
        if level1:
            c1.out_mid1, c1.out_skip1, c1.out_pool2 = (t.data_ptr() for t in sets[1, j][1])
            c1.out_z[:] = (span1[0] + SHIFT // 2, span1[1] + SHIFT // 2)
            c1.out_shift = SHIFT // 2
    if j == 1:
        y.in_y[:] = YC
    else:
        y.out_skip_y, y.out_pool_y = (t.data_ptr() for t in sets[k, 1][0])
        y.out_y[:] = (YC[0] + SHIFT, YC[1] + SHIFT)
        y.out_shift_y = SHIFT
        if k == 0:
            y.out_skip_d, y.out_pool_d = (t.data_ptr() for t in sets[1, 1][0])
    if event is not None:
        y.encoder_event = event
    return c, c1, y


def _chain(S, dev, fill, level1):  # noqa: F811
    """The four batches in plan order -> {(k, j): kept output}, and whether every guard band survived."""
    model, lib = S["model"], _native.lib()
    d, h, w = PATCH
    raws, sets = [], {}
    for kj in ORDER:
        pair = [_guarded(2 * e, fill, dev) for e in model.carry_pair_elems((2,) + PATCH)]
        triple = [_guarded(2 * e, fill, dev) for e in model.carry_triple_elems((2,) + PATCH)]
        raws += [r for r, _ in pair + triple]
        sets[kj] = ([t for _, t in pair], [t for _, t in triple])
    ws_raw, ws = _guarded(S["need"], fill, dev)
    numel = 2 * 3 * d * h * w
    got = {}
    for k, j in ORDER:
        out_raw, out = _guarded(4 * numel, SENTINEL, dev)
        c, c1, y = _structs(S, dev, sets, k, j, level1)
        ws.fill_(fill)      # (a batch must not depend on what the one before left in the workspace)
        rc = lib.exaspim_unet_forward_prepared_carry_y(
            S["handle"], S["prepared"][k, j].data_ptr(), out.data_ptr(), 2, d, h, w, 1, TRIM, STRIDE, S["keep_hi"],
            ctypes.byref(c), ctypes.byref(c1) if c1 is not None else None, ctypes.byref(y), ws.data_ptr(), S["need"],
            torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, _native.last_error()
        assert _intact(out_raw, SENTINEL)
        got[k, j] = out.view(torch.float32).view(2, 3, d, h, w).cpu()
    return got, all(_intact(r, fill) for r in raws) and _intact(ws_raw, fill)


@pytest.mark.parametrize("level1", [True, False], ids=["carry1", "carry"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_four_batches_equal_each_alone_and_the_chain_without_rows(state, dev, dtype, level1):  # noqa: F811
    S = _setup(state, dev, dtype)
    model, lib = S["model"], _native.lib()
    assert model.carry_planes((2,) + PATCH, STRIDE, SHIFT, dev) == ZC
    assert model.carry_rows((2,) + PATCH, STRIDE, SHIFT, dev) == YC == inference._carry_rows_span(PATCH[1], SHIFT)
    assert model.carry_rows((16, 96, 96, 96), 64, 64, dev) == (8, 24)
    kept = torch.zeros((2, 3) + PATCH, dtype=torch.bool)
    kept[(Ellipsis,) + tuple(slice(TRIM, p - TRIM) for p in PATCH)] = True
    try:
        _native.check(lib.exaspim_unet_set_options(S["handle"], _native.OPT_CARRY_NO_ROWS), "set_options")
        assert model.carry_rows((2,) + PATCH, STRIDE, SHIFT, dev) == (0, 0)
        no_rows, intact = _chain(S, dev, FILLS[1], level1)
    finally:
        _native.check(lib.exaspim_unet_set_options(S["handle"], 0), "set_options")
    assert intact
    for fill in FILLS:
        got, intact = _chain(S, dev, fill, level1)
        assert intact, f"fill {fill:#x}: a guard band"
        for kj in ORDER:
            for want, what in ((S["want"][kj], "the batch alone"), (no_rows[kj], "EXASPIM_OPT_CARRY_NO_ROWS")):
                differ = got[kj].view(torch.int32)[kept] != want.view(torch.int32)[kept]
                assert not differ.any(), (f"batch {kj}, fill {fill:#x} against {what}: {int(differ.sum())} of "
                                          f"{int(kept.sum())} kept voxels differ, first at "
                                          f"{kept.nonzero()[differ][:4].tolist()}")
            assert not bool(torch.isnan(got[kj][kept]).any())
            assert bool((got[kj].view(torch.int32)[~kept] == SENTINEL_WORD).all()), "voxels outside the kept box were written"


def test_the_event_is_recorded_after_the_first_level(state, dev):  # noqa: F811
    S = _setup(state, dev, "fp16")
    model, lib = S["model"], _native.lib()
    d, h, w = PATCH
    sets = {kj: ([torch.zeros(e, dtype=torch.int16, device=dev) for e in model.carry_pair_elems((2,) + PATCH)], None)
            for kj in ORDER}
    ws = torch.zeros(S["need"], dtype=torch.uint8, device=dev)
    out = torch.empty((2, 3, d, h, w), dtype=torch.float32, device=dev)
    event = torch.cuda.Event()
    event.record()
    c, _, y = _structs(S, dev, sets, 0, 0, False, event=event.cuda_event)
    other = torch.cuda.Stream(dev)
    rc = lib.exaspim_unet_forward_prepared_carry_y(
        S["handle"], S["prepared"][0, 0].data_ptr(), out.data_ptr(), 2, d, h, w, 1, TRIM, STRIDE, S["keep_hi"],
        ctypes.byref(c), None, ctypes.byref(y), ws.data_ptr(), S["need"], torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _native.last_error()
    other.wait_event(event)
    with torch.cuda.stream(other):      # what the y successor sees once the event has fired
        rows = sets[0, 1][0][0].clone()
    torch.cuda.synchronize()
    assert bool((rows != 0).any()), "the y successor's rows were not stored before the event"


BAD = {
    "in_y not whole tiles": dict(in_y=(8, 20)),
    "in_y beyond h - 2": dict(in_y=(56, 64)),
    "out_y not the range of the shift": dict(out_y=(40, 48)),
    "one y target": dict(one=True),
    "out_y overlaps in_y": dict(in_y=(8, 48)),
    "diagonal without the z carry out": dict(no_z=True),
    "reserved": dict(reserved=1),
}


@pytest.mark.parametrize("what", list(BAD))
def test_requests_the_engine_cannot_honour_are_refused(state, dev, what):  # noqa: F811
    S = _setup(state, dev, "fp16")
    model, lib = S["model"], _native.lib()
    d, h, w = PATCH
    kw = BAD[what]
    raws, sets = [], {}
    for kj in ORDER:
        pair = [_guarded(2 * e, SENTINEL, dev) for e in model.carry_pair_elems((2,) + PATCH)]
        raws += [r for r, _ in pair]
        sets[kj] = ([t for _, t in pair], None)
    c, _, y = _structs(S, dev, sets, 0, 0, False)
    if "in_y" in kw:
        y.in_y[:] = kw["in_y"]
    if "out_y" in kw:
        y.out_y[:] = kw["out_y"]
    if kw.get("one"):
        y.out_pool_y = None
    if kw.get("no_z"):
        c.out_skip = c.out_pool = None
        c.out_z[:] = (0, 0)
        c.out_shift = 0
    y.reserved = kw.get("reserved", 0)
    ws_raw, ws = _guarded(S["need"], SENTINEL, dev)
    out_raw, out = _guarded(4 * 2 * 3 * d * h * w, SENTINEL, dev)
    rc = lib.exaspim_unet_forward_prepared_carry_y(
        S["handle"], S["prepared"][0, 0].data_ptr(), out.data_ptr(), 2, d, h, w, 1, TRIM, STRIDE, S["keep_hi"],
        ctypes.byref(c), None, ctypes.byref(y), ws.data_ptr(), S["need"], torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and "forward:" in _native.last_error(), (rc, _native.last_error())
    for raw in raws + [ws_raw, out_raw]:        # refused before anything was launched
        assert bool((raw == SENTINEL).all())


# 2 x 2 starts along z and y, rows of three, every high face ragged; and a y stride of 16 under a height of 64,
# where a batch takes rows [8, 40) over and would have to pass on [24, 56): the y chain is cut at every second row
PREDICT = {
    "ragged": ((90, 85, 100), dict(batch_size=3, patch_shape=PATCH, overlap=(32, 32, 32), trim=TRIM)),
    "cut y chain": ((90, 106, 90), dict(batch_size=2, patch_shape=PATCH, overlap=(32, 48, 32), trim=TRIM)),
}


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(PREDICT))
def test_predict_is_the_same_with_rows_carried_and_not(state, dev, dtype, name, monkeypatch):  # noqa: F811
    model = _setup(state, dev, dtype)["model"]
    shape, kw = PREDICT[name]
    vol = inference.DeviceVolume.from_array(synthetic.synth_volume(shape, seed=61), dev)
    calls = []
    run_prepared = model.run_prepared

    def logging(*args, **kwargs):
        c = kwargs.get("carry") or {}
        calls.append((tuple(c.get("in_y") or (0, 0)), c.get("out_y_pair") is not None, c.get("out_d_pair") is not None,
                      c.get("encoder_event") is not None))
        return run_prepared(*args, **kwargs)

    monkeypatch.setattr(model, "run_prepared", logging)
    assert model.engine_options == 0 and inference.CARRY_Z and inference.ROWS_CARRY_Y
    monkeypatch.setattr(inference, "ROWS_CARRY_Y", False)
    want = inference.predict(vol, model, verbose=False, n_streams=1, **kw)
    assert calls and not any(c[0] != (0, 0) or c[1] or c[2] for c in calls)
    monkeypatch.setattr(inference, "ROWS_CARRY_Y", True)
    rows = (8, 24) if name == "ragged" else (8, 40)
    for n_streams in (1, 3):
        del calls[:]
        got = inference.predict(vol, model, verbose=False, n_streams=n_streams, **kw)
        assert sum(c[0] == rows for c in calls) == sum(c[1] for c in calls) > 0, calls
        assert any(c[2] for c in calls), calls      # (a diagonal block in both plans)
        assert all(c[3] == (n_streams > 1) for c in calls if c[1]), calls
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, n_streams)
    # a pool that admits the z links' sets and not one more: the planes are carried, the rows are not
    starts = list(inference.generate_patch_starts((1, 1) + shape, kw["patch_shape"], kw["overlap"]))
    succ = inference.carry_plan(starts, kw["batch_size"], kw["patch_shape"], kw["overlap"])
    _, peak, level1 = inference._carry_schedule(model, succ, starts, kw["batch_size"], kw["patch_shape"], kw["overlap"], 1, dev)
    shape4 = (kw["batch_size"],) + tuple(kw["patch_shape"])
    per_set = 2 * sum(model.carry_pair_elems(shape4)) + (2 * sum(model.carry_triple_elems(shape4)) if level1 else 0)
    if name == "ragged":
        monkeypatch.setattr(inference, "CARRY_POOL_BYTES", peak * per_set)
        del calls[:]
        got = inference.predict(vol, model, verbose=False, n_streams=1, **kw)
        assert calls and not any(c[0] != (0, 0) or c[1] or c[2] for c in calls), calls
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "under the cap"
