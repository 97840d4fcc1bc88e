"""
exaspim_unet_forward_prepared_clipped: the trimmed forward for a batch whose patches reach beyond the
volume's high faces. The caller keeps local [trim, keep_hi) per axis; the level-0 decoder (the upsampling,
up4.0 with its thin remainders, up4.3 with the fused head) runs on the clipped region only.

Held to exaspim_unet_forward_prepared(_row) on the same input, on workspaces this file fills first (the
fills of test_gpu_workspace): inside the kept box the bits are equal, outside it the output keeps its
sentinel, the guards behind the workspace and the output stay as they were, and the four fills agree.
The production corner is also held to golden g4 inside the box. predict() on a volume whose last z and y
rows are partial gives the bits of the same call with inference.CLIP_TO_VOLUME = False.
"""

import numpy as np
import pytest
import torch

import test_gpu_workspace as W
from aind_exaspim_neuron_segmentation_amd import _native, inference
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from test_gpu_workspace import dev, oracle, state  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# (case of test_gpu_workspace.CASES, trim, keep_hi): the smallest shapes at which each mechanism is live
CLIPS = [
    (2, 8, (24, 24, 40)),   # (32,32,48) x 2: unclipped, equal to the trimmed entry everywhere
    (2, 8, (9, 24, 40)),    # one kept plane
    (2, 8, (17, 19, 40)),   # odd extents, masked z tile, up4.0 y extent 13
    (2, 8, (24, 24, 26)),   # x clipped
    (2, 8, (24, 22, 40)),   # up4.0 extent 16 on y: the y remainder disappears, x keeps its own (34 = 2 x 16 + 2)
    (7, 4, (9, 12, 92)),    # (16,16,96) x 2, row stride 64: row mode with a clip
    (1, 8, (64, 64, 88)),   # (96,96,96): the production corner, up4.0 extent 58 = 7 x 8 + 2 on y
]


def _call_clipped(lib, handle, inp, layout, out, n, patch, trim, row_stride, keep_hi, ws, ws_bytes, dev):  # noqa: F811
    d, h, w = patch
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.exaspim_unet_forward_prepared_clipped(handle, W._prepared(inp, layout, patch, dev).data_ptr(),
                                                   out.data_ptr(), n, d, h, w, 1, trim, row_stride,
                                                   _native.int3(keep_hi), ws.data_ptr(), ws_bytes, stream)
    torch.cuda.synchronize()
    return rc


def _run_clipped(state, dev, model, case, trim, keep_hi, fill):  # noqa: F811
    """test_gpu_workspace._run for the clipped entry."""
    lib = _native.lib()
    patch, n, row_stride = W.CASES[case]
    d, h, w = patch
    handle = model._ensure_engine(dev)
    layout = model.input_layout(dev)
    need = lib.exaspim_unet_workspace_bytes(handle, n, d, h, w)
    assert need, _native.last_error()
    if fill == "stale":
        big = lib.exaspim_unet_workspace_bytes(handle, n + 1, d, h, w)
        assert big >= need + W.GUARD
        ws = torch.empty(big, dtype=torch.uint8, device=dev)
        ws.fill_(0xA5)
        other = W._inputs(state, dev, case, n + 1, W.SEED[case] + 1000)
        scratch = torch.empty((n + 1, model.output_channels, d, h, w), dtype=torch.float32, device=dev)
        _native.check(_call_clipped(lib, handle, other, layout, scratch, n + 1, patch, trim, row_stride, keep_hi, ws,
                                    big, dev), "clipped")
        del scratch
    else:
        ws = torch.empty(need + W.GUARD, dtype=torch.uint8, device=dev)
        ws.fill_(int(fill, 16))
    ws_guard = ws[need: need + W.GUARD].clone()
    numel = n * model.output_channels * d * h * w
    out = torch.empty(numel + W.GUARD // 4, dtype=torch.float32, device=dev)
    out.view(torch.uint8).fill_(W.SENTINEL)
    inp = W._inputs(state, dev, case, n, W.SEED[case])
    _native.check(_call_clipped(lib, handle, inp, layout, out, n, patch, trim, row_stride, keep_hi, ws, need, dev),
                  "clipped")
    assert torch.equal(ws[need: need + W.GUARD], ws_guard), f"{fill}: bytes behind workspace_bytes were written"
    assert bool((W._bits(out[numel:]) == W.SENTINEL_WORD).all()), f"{fill}: bytes behind the output were written"
    return out[:numel].view(n, model.output_channels, d, h, w).cpu()


def _check_clipped(state, dev, golden, dtype, case, trim, keep_hi, variant="base"):  # noqa: F811
    model, _ = W._model(state, dev, dtype, variant)
    patch, n, row_stride = W.CASES[case]
    what = f"case {case} {dtype} {variant} trim {trim} keep_hi {keep_hi}"
    want = W._run(state, dev, model, "row" if row_stride else "prepared", case, trim, "0x00")
    kept = torch.zeros((n, model.output_channels) + patch, dtype=torch.bool)
    kept[(Ellipsis,) + tuple(slice(trim, k) for k in keep_hi)] = True
    for fill in W.FILLS:
        got = _run_clipped(state, dev, model, case, trim, keep_hi, fill)
        differ = W._bits(got)[kept] != W._bits(want)[kept]
        if differ.any():
            where = kept.nonzero()[differ][:4].tolist()
            raise AssertionError(f"{what}, fill {fill}: {int(differ.sum())} of {int(kept.sum())} kept voxels differ "
                                 f"from the trimmed entry, first at {where}")
        written = int((W._bits(got)[~kept] != W.SENTINEL_WORD).sum())
        assert written == 0, f"{what}, fill {fill}: {written} of {int((~kept).sum())} voxels outside the box were written"
    if case == 1:
        ref = torch.from_numpy(golden("g4_single_patch.npz")["sigmoid_sub"].copy())[None]
        k = kept[..., ::8, ::8, ::8]
        err = float((got[..., ::8, ::8, ::8] - ref).abs()[k].max())
        print(f"{what}: vs golden g4 inside the box: {err:.3e} over {int(k.sum())} voxels (tolerance {W.PROB_TOL[dtype]:.1e})")
        assert err < W.PROB_TOL[dtype]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case,trim,keep_hi", CLIPS)
def test_clipped_equals_trimmed_inside_the_box(state, dev, golden, case, trim, keep_hi, dtype):  # noqa: F811
    if W.CASES[case][2]:
        W._assert_row_mode(case, dtype)
    _check_clipped(state, dev, golden, dtype, case, trim, keep_hi)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("variant", W.ROW_VARIANTS)
def test_clipped_row_mode_on_model_variants(state, dev, golden, variant, dtype):  # noqa: F811
    """Row mode with a clip on 1, 2 and 4 outputs, ConvTranspose3d up blocks and widths 0.75 and 0.5."""
    model, _ = W._model(state, dev, dtype, variant)
    W._assert_row_mode(7, dtype, model.channels)
    _check_clipped(state, dev, golden, dtype, 7, 4, (9, 12, 92), variant)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_clipped_float32_storage(state, dev, golden, dtype):  # noqa: F811
    _check_clipped(state, dev, golden, dtype, 2, 8, (17, 19, 40))


@pytest.mark.parametrize("keep_hi", [(8, 24, 40), (24, 0, 40), (24, 24, 8), (25, 24, 40), (24, 24, 41), (24, 33, 40)])
def test_invalid_keep_hi_is_rejected(state, dev, keep_hi):  # noqa: F811
    model, _ = W._model(state, dev, "fp16", "base")
    lib = _native.lib()
    patch, n, _ = W.CASES[2]
    handle = model._ensure_engine(dev)
    need = lib.exaspim_unet_workspace_bytes(handle, n, *patch)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = torch.zeros((n, 3) + patch, dtype=torch.float32, device=dev)
    inp = W._inputs(state, dev, 2, n, W.SEED[2])
    rc = _call_clipped(lib, handle, inp, model.input_layout(dev), out, n, patch, 8, 0, keep_hi, ws, need, dev)
    assert rc == -1, (rc, _native.last_error())   # EXASPIM_E_INVALID
    assert "keep_hi" in _native.last_error()
    assert not bool(out.any())


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_predict_with_partial_last_rows_equals_the_unclipped_plan(state, dev, dtype):  # noqa: F811
    """160 x 160 x 224 under patches of (32, 32, 96), overlap (8, 8, 32), trim 4: the last z and y starts
    (144) keep [4, 16) of [4, 28); x ends exactly (128 + 96), and a batch is one row along x (row mode in
    the 16-bit modes). Same bits with and without the clip."""
    model, _ = W._model(state, dev, dtype, "base")
    vol = synthetic.synth_volume((160, 160, 224), seed=31)
    kw = dict(batch_size=3, patch_shape=(32, 32, 96), overlap=(8, 8, 32), trim=4, verbose=False)
    plan = inference.SlidingWindow(vol.shape, kw["patch_shape"], kw["overlap"], kw["trim"])
    starts = plan.starts()
    hi = [inference.batch_keep_hi(starts[i:i + 3], kw["patch_shape"], 4, vol.shape) for i in range(0, len(starts), 3)]
    assert (16, 28, 92) in hi and (28, 16, 92) in hi and (16, 16, 92) in hi and None in hi
    assert inference.CLIP_TO_VOLUME
    got = inference.predict(vol, model, **kw)
    inference.CLIP_TO_VOLUME = False
    try:
        want = inference.predict(vol, model, **kw)
    finally:
        inference.CLIP_TO_VOLUME = True
    assert got.shape == want.shape == (3, 160, 160, 224)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
