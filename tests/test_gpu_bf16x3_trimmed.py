"""
compute_dtype="bf16x3" with the head fused into up4.3 and the trimmed forward (engine.hip): the
margin of a trimmed forward is left untouched, every kept voxel has the bits of the full forward,
and the fused plan gives the bits of the separate-head plan (EXASPIM_OPT_SEPARATE_HEAD: the head as
a launch of its own over the whole patch, nothing trimmed) -- through the C entry points, through
predict() / predict_streaming() and against the reference's goldens with the tolerances of
test_gpu_bf16x3.py.
"""

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from test_gpu_bf16x3 import LOGITS_TOL, PROB_TOL, dev, make_model, normalized_input, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _forward(model, x, sig=1, trim=None, fill=float("nan"), absmax=False):
    """exaspim_unet_forward, _forward_trimmed or _forward_absmax on a caller-filled output."""
    lib = _native.lib()
    n, _, d, h, w = x.shape
    handle = model._ensure_engine(x.device)
    need = lib.exaspim_unet_workspace_bytes(handle, n, d, h, w)
    assert need, _native.last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    out = torch.full((n, model.output_channels, d, h, w), fill, dtype=torch.float32, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if absmax:
        slots = torch.zeros(22, dtype=torch.float32, device=x.device)
        rc = lib.exaspim_unet_forward_absmax(handle, x.data_ptr(), out.data_ptr(), n, d, h, w, sig,
                                             slots.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    elif trim is None:
        rc = lib.exaspim_unet_forward(handle, x.data_ptr(), out.data_ptr(), n, d, h, w, sig, ws.data_ptr(),
                                      ws.numel(), stream)
    else:
        rc = lib.exaspim_unet_forward_trimmed(handle, x.data_ptr(), out.data_ptr(), n, d, h, w, sig, trim,
                                              ws.data_ptr(), ws.numel(), stream)
    _native.check(rc, "forward")
    torch.cuda.synchronize()
    return out.cpu()


# ---- the trimmed forward ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,trim,fill", [((96, 96, 96), 8, float("nan")), ((32, 48, 64), 4, -7.0),
                                             ((32, 32, 32), 1, float("nan")), ((16, 48, 32), 3, -7.0)])
def test_trimmed_forward_leaves_the_margin_untouched(dev, oracle, shape, trim, fill):  # noqa: F811
    model, _ = make_model(dev)
    n = 1 if shape[0] == 96 else 2
    x = normalized_input(oracle, shape, seed=90, n=n).to(dev)
    full = _forward(model, x)
    part = _forward(model, x, trim=trim, fill=fill)
    assert not torch.isnan(full).any()
    kept = torch.zeros(full.shape, dtype=torch.bool)
    kept[(slice(None), slice(None)) + tuple(slice(trim, s - trim) for s in shape)] = True
    assert torch.equal(_bits(full)[kept], _bits(part)[kept]), "a kept voxel differs from the full forward"
    want_fill = _bits(torch.full((1,), fill))[0]
    written = int((_bits(part)[~kept] != want_fill).sum())
    assert written == 0, f"{written} of {int((~kept).sum())} margin voxels were written"


def test_a_trim_that_leaves_nothing_runs_the_full_forward(dev, oracle):  # noqa: F811
    model, _ = make_model(dev)
    x = normalized_input(oracle, (16, 16, 16), seed=91, n=2).to(dev)
    full = _forward(model, x)
    part = _forward(model, x, trim=8)
    assert not torch.isnan(full).any()
    assert torch.equal(_bits(full), _bits(part))


# ---- fused against separate head -------------------------------------------------------------
@pytest.mark.parametrize("oc,trilinear,wm,shape", [(3, True, 1, (32, 48, 32)), (1, True, 1, (16, 32, 48)),
                                                   (3, False, 1, (32, 32, 48)), (3, True, 0.5, (32, 48, 16)),
                                                   (1, True, 0.125, (16, 16, 64))])
def test_fused_head_has_the_bits_of_the_separate_head(dev, oracle, oc, trilinear, wm, shape):  # noqa: F811
    model, _ = make_model(dev, out_channels=oc, seed=5, trilinear=trilinear, wm=wm)
    x = normalized_input(oracle, shape, seed=92, n=3).to(dev)
    for sig in (0, 1):
        model.engine_options = 0
        fused = _forward(model, x, sig=sig)
        probe = _forward(model, x, sig=sig, absmax=True)     # keeps the separate head and the full pass
        model.engine_options = _native.OPT_SEPARATE_HEAD
        separate = _forward(model, x, sig=sig)
        trimmed_separate = _forward(model, x, sig=sig, trim=4, fill=-7.0)   # nothing is trimmed then
        model.engine_options = 0
        assert not torch.isnan(fused).any()
        assert torch.equal(_bits(fused), _bits(separate)), f"sig={sig}"
        assert torch.equal(_bits(fused), _bits(probe)), f"sig={sig} (forward_absmax)"
        assert torch.equal(_bits(fused), _bits(trimmed_separate)), f"sig={sig} (trimmed entry, separate head)"


# ---- end to end ------------------------------------------------------------------------------
def test_predict_default_geometry_160(dev, golden):  # noqa: F811
    from aind_exaspim_neuron_segmentation_amd import inference

    g = golden("g6_default_160.npz")
    vol = synthetic.synth_volume((160, 160, 160), seed=0)
    model, _ = make_model(dev)
    got = inference.predict(vol, model, batch_size=3, verbose=False)      # 8 patches: 3 + 3 + 2
    err = np.abs(got[:, ::5, ::5, ::5] - g["pred_sub"]).max()
    err2 = np.abs(got[:, 80, 81, :] - g["pred_line"]).max()
    print(f"bf16x3 trimmed predict 160^3 defaults vs reference: {err:.3e} / {err2:.3e}")
    assert err < PROB_TOL and err2 < PROB_TOL
    streamed = inference.predict_streaming(vol, model, batch_size=3, verbose=False)
    np.testing.assert_array_equal(streamed, got)
    del streamed
    model.engine_options = _native.OPT_SEPARATE_HEAD
    want = inference.predict(vol, model, batch_size=3, verbose=False)
    model.engine_options = 0
    np.testing.assert_array_equal(got, want)


def test_predict_ragged_small_patches(dev, golden):  # noqa: F811
    from aind_exaspim_neuron_segmentation_amd import inference

    g = golden("g5_fullwidth_small.npz")
    vol = synthetic.synth_volume((72, 40, 56), seed=11)
    model, _ = make_model(dev)
    kw = dict(batch_size=4, patch_shape=(32, 32, 32), overlap=(8, 8, 8), trim=4)
    got = inference.predict(vol, model, verbose=False, **kw)
    err = np.abs(got[:, ::2, ::2, ::2] - g["pred"]).max()
    print(f"bf16x3 trimmed predict 72x40x56 vs reference: {err:.3e}")
    assert err < PROB_TOL
    streamed = inference.predict_streaming(vol, model, verbose=False, **kw)
    np.testing.assert_array_equal(streamed, got)
    model.engine_options = _native.OPT_SEPARATE_HEAD
    want = inference.predict(vol, model, verbose=False, **kw)
    model.engine_options = 0
    np.testing.assert_array_equal(got, want)
    # one output channel, another overlap and trim, a short last batch
    model1, _ = make_model(dev, out_channels=1, seed=4)
    kw1 = dict(batch_size=5, patch_shape=(32, 32, 32), overlap=(16, 16, 16), trim=2)
    got1 = inference.predict(vol, model1, affinity_mode=False, verbose=False, **kw1)
    assert np.abs(got1[::2, ::2, ::2] - g["pred_fg"]).max() < PROB_TOL
    model1.engine_options = _native.OPT_SEPARATE_HEAD
    want1 = inference.predict(vol, model1, affinity_mode=False, verbose=False, **kw1)
    np.testing.assert_array_equal(got1, want1)


def test_logits_meet_the_single_patch_golden_on_both_plans(dev, oracle, golden):  # noqa: F811
    g = golden("g4_single_patch.npz")
    model, _ = make_model(dev)
    x = normalized_input(oracle, (96, 96, 96), seed=0).to(dev)
    outs = []
    for opt in (0, _native.OPT_SEPARATE_HEAD):
        model.engine_options = opt
        got = model(x).cpu()
        outs.append(got)
        err = np.abs(got.numpy()[0][:, ::8, ::8, ::8] - g["logits_sub"]).max()
        err2 = np.abs(got.numpy()[0][:, 40:44, 17:21, :] - g["logits_slab"]).max()
        print(f"bf16x3 96^3 logits vs reference, options {opt}: {err:.3e} / {err2:.3e}")
        assert err < LOGITS_TOL and err2 < LOGITS_TOL
    model.engine_options = 0
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


# ---- the option bit --------------------------------------------------------------------------
def test_set_options_accepts_the_new_bit_only(dev):  # noqa: F811
    lib = _native.lib()
    model, _ = make_model(dev)
    handle = model._ensure_engine(dev)
    assert _native.OPT_SEPARATE_HEAD == 64
    assert lib.exaspim_unet_set_options(handle, 64) == 0
    assert lib.exaspim_unet_set_options(handle, 64 | 1) == 0
    assert lib.exaspim_unet_set_options(handle, 128) == -1 and "unknown option" in _native.last_error()
    assert lib.exaspim_unet_set_options(handle, 0) == 0
