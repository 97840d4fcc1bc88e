"""
GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through
the C ABI, against the CPU oracle on the same seeded inputs and against the
golden vectors produced by the reference itself.

Tolerances: integer / index / byte work (percentiles, gather, stitch) is
bit-exact; the fp32 network path is held to 3e-5 abs on logits (measured 3e-6) and 5e-6 abs on
probabilities (north_star allows 1e-3); the 16-bit mode that bench.py runs
(fp16 storage, fp32 accumulate) is held to north_star's 1e-3 on the maximum;
bf16 storage (8 significant bits) is held to 4e-3 (measured 2.3e-3 .. 2.9e-3)
and is not the benchmarked mode. All weights are seeded random weights (no
checkpoint ships with the reference): 16-bit parity on trained weights is
unpinned.
"""

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd.utils import synthetic

pytestmark = pytest.mark.gpu

PROB_TOL_FP32 = 5e-6                              # probabilities of the fp32 path (max abs)
PROB_TOL_16BIT = [("bf16", 4e-3), ("fp16", 1e-3)]   # ... and of the 16-bit storage modes


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle():
    from oracle import reference_path

    return reference_path


def make_model(dev, out_channels=3, seed=1, compute_dtype="fp32", trilinear=True):
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(out_channels, 1, seed=seed, trilinear=trilinear)
    model = UNet3D(output_channels=out_channels, trilinear=trilinear,
                   compute_dtype=compute_dtype)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return model.to(dev).eval(), sd


def normalized_input(oracle, shape, seed, n=1):
    vols = [synthetic.synth_volume(shape, seed=seed + i) for i in range(n)]
    x = np.stack([oracle.normalize(np.minimum(v, 1000)) for v in vols])[:, None]
    return torch.tensor(x.astype(np.float32))


# ---------------------------------------------------------------- network ---
@pytest.mark.parametrize("shape", [(32, 32, 32), (16, 48, 64), (48, 32, 16)])
def test_unet_logits_fp32_vs_oracle(dev, oracle, shape):
    model, sd = make_model(dev)
    x = normalized_input(oracle, shape, seed=40, n=2)
    want = oracle.unet_forward(x, oracle.OracleModel(sd).sd).numpy()
    got = model(x.to(dev)).cpu().numpy()
    assert got.shape == want.shape
    err = np.abs(got - want).max()
    print(f"fp32 logits {shape}: max|diff| = {err:.3e}")
    assert err < 3e-5


def test_unet_single_96_patch_vs_reference_golden(dev, oracle, golden):
    g = golden("g4_single_patch.npz")
    model, _ = make_model(dev)
    x = normalized_input(oracle, (96, 96, 96), seed=0)
    logits = model(x.to(dev))
    got = logits.cpu().numpy()[0]
    err = np.abs(got[:, ::8, ::8, ::8] - g["logits_sub"]).max()
    err2 = np.abs(got[:, 40:44, 17:21, :] - g["logits_slab"]).max()
    print(f"fp32 96^3 logits vs reference: {err:.3e} / {err2:.3e}")
    assert err < 3e-5 and err2 < 3e-5
    sig = torch.sigmoid(logits).cpu().numpy()[0, :, ::8, ::8, ::8]
    assert np.abs(sig - g["sigmoid_sub"]).max() < PROB_TOL_FP32


@pytest.mark.parametrize("cdt,tol", PROB_TOL_16BIT)
def test_unet_16bit_paths_vs_oracle(dev, oracle, cdt, tol):
    # 16-bit storage of activations/weights, fp32 accumulate: tolerance on the
    # probabilities (max abs): fp16 = north_star's 1e-3; bf16 has 8 significant bits.
    model, sd = make_model(dev, compute_dtype=cdt)
    x = normalized_input(oracle, (32, 32, 32), seed=41, n=2)
    want = torch.sigmoid(oracle.unet_forward(x, oracle.OracleModel(sd).sd)).numpy()
    got = model.run(x.to(dev), apply_sigmoid=True).cpu().numpy()
    err = np.abs(got - want)
    print(f"{cdt} probabilities: max {err.max():.3e} mean {err.mean():.3e} "
          f"p99.9 {np.quantile(err, 0.999):.3e}")
    assert err.max() < tol


def test_conv_transpose_variant_vs_reference_golden_and_oracle(dev, oracle, golden):
    """UNet3D(trilinear=False): ConvTranspose3d(k=2, s=2) up blocks (unet3d.py:254-258)."""
    from aind_exaspim_neuron_segmentation_amd import inference

    g = golden("g7_conv_transpose.npz")
    model, sd = make_model(dev, seed=8, trilinear=False)
    x = normalized_input(oracle, (32, 32, 48), seed=60, n=2)
    got = model(x.to(dev)).cpu().numpy()
    want = oracle.unet_forward(x, oracle.OracleModel(sd).sd).numpy()
    e_ref = max(np.abs(got[:, :, ::2, ::2, ::2] - g["logits_sub"]).max(),
                np.abs(got[1, :, 17, 9, :] - g["logits_row"]).max())
    e_orc = np.abs(got - want).max()
    print(f"convT fp32 logits: vs reference {e_ref:.3e}, vs oracle {e_orc:.3e}")
    assert e_ref < 3e-5 and e_orc < 3e-5
    vol = synthetic.synth_volume((56, 40, 48), seed=61)
    pred = inference.predict(vol, model, batch_size=3, patch_shape=(32, 32, 32),
                             overlap=(8, 8, 8), trim=4, verbose=False)
    e_pred = np.abs(pred[:, ::2, ::2, ::2] - g["pred_sub"]).max()
    print(f"convT fp32 predict vs reference: {e_pred:.3e}")
    assert e_pred < 5e-6


@pytest.mark.parametrize("cdt,tol", PROB_TOL_16BIT)
def test_conv_transpose_variant_16bit(dev, oracle, cdt, tol):
    model, sd = make_model(dev, seed=8, compute_dtype=cdt, trilinear=False)
    x = normalized_input(oracle, (32, 32, 32), seed=62, n=3)
    want = torch.sigmoid(oracle.unet_forward(x, oracle.OracleModel(sd).sd)).numpy()
    got = model.run(x.to(dev), apply_sigmoid=True).cpu().numpy()
    err = np.abs(got - want)
    print(f"convT {cdt} probabilities: max {err.max():.3e} mean {err.mean():.3e} "
          f"p99.9 {np.quantile(err, 0.999):.3e}")
    assert err.max() < tol


def test_conv_transpose_half_width(dev, oracle):
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(1, 0.5, seed=4, trilinear=False)
    model = UNet3D(output_channels=1, trilinear=False, width_multiplier=0.5)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = model.to(dev).eval()
    x = normalized_input(oracle, (16, 32, 16), seed=63, n=2)
    want = oracle.unet_forward(x, oracle.OracleModel(sd).sd).numpy()
    got = model(x.to(dev)).cpu().numpy()
    assert np.abs(got - want).max() < 5e-5


@pytest.mark.parametrize("cdt", ["fp32", "bf16"])
@pytest.mark.parametrize("shape,trim", [((96, 96, 96), 8), ((32, 48, 64), 4), ((32, 32, 32), 1),
                                        ((16, 16, 16), 7)])
def test_trimmed_forward_is_bit_identical_inside(dev, oracle, cdt, shape, trim):
    """exaspim_unet_forward_trimmed skips work only the discarded margin needs:
    every voxel predict() keeps (inference.py:161-162) must not change by a bit."""
    model, _ = make_model(dev, compute_dtype=cdt)
    x = normalized_input(oracle, shape, seed=70, n=2).to(dev)
    full = model.run(x, apply_sigmoid=True)
    out = torch.full_like(full, -7.0)
    part = model.run(x, apply_sigmoid=True, out=out, trim=trim)
    inner = (Ellipsis,) + (slice(trim, -trim),) * 3
    assert torch.equal(part[inner], full[inner])
    # the margin is left untouched (predict never reads it)
    assert bool((part[..., 0, :, :] == -7.0).all()) and bool((part[..., :, :, -1] == -7.0).all())


def test_trimmed_forward_variants(dev, oracle):
    """Trim on the ConvTranspose variant and on fp16, a batch that does not fill the
    persistent grid evenly, and a trim that would leave nothing (= full forward)."""
    model, _ = make_model(dev, seed=8, compute_dtype="fp16", trilinear=False)
    x = normalized_input(oracle, (32, 32, 48), seed=71, n=5).to(dev)
    full = model.run(x, apply_sigmoid=True)
    part = model.run(x, apply_sigmoid=True, trim=6)
    assert torch.equal(part[..., 6:-6, 6:-6, 6:-6], full[..., 6:-6, 6:-6, 6:-6])
    small = normalized_input(oracle, (16, 16, 16), seed=72, n=1).to(dev)
    assert torch.equal(model.run(small, trim=8), model.run(small))
    with pytest.raises(ValueError, match="negative trim"):
        model.run(small, trim=-1)


def test_fused_pool_matches_oracle_stages(dev, oracle, golden):
    """inc.3 writes its own max-pool: the full-width 96^3 golden (per-stage features of the
    reference) pins everything downstream of it; here a ragged batch at small sizes."""
    model, sd = make_model(dev, seed=3)
    for shape, n in (((16, 32, 16), 3), ((48, 16, 32), 1)):
        x = normalized_input(oracle, shape, seed=73, n=n)
        want = oracle.unet_forward(x, oracle.OracleModel(sd).sd).numpy()
        got = model(x.to(dev)).cpu().numpy()
        assert np.abs(got - want).max() < 5e-5


@pytest.mark.parametrize("wm,shape,n", [(3, (16, 16, 32), 1), (0.25, (32, 16, 16), 2), (1, (16, 16, 16), 33)])
def test_width_multipliers_and_large_batches(dev, oracle, wm, shape, n):
    """96-channel level 0 (three 32-cout slices per tile in the z-column kernel, no fused
    head or pool), heavily padded narrow networks, and a batch beyond the benchmark's."""
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(2, wm, seed=11)
    model = UNet3D(output_channels=2, width_multiplier=wm)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = model.to(dev).eval()
    x = normalized_input(oracle, shape, seed=74, n=n)
    want = oracle.unet_forward(x, oracle.OracleModel(sd).sd).numpy()
    got = model(x.to(dev)).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"width x{wm}, batch {n}: max|diff| = {err:.3e}")
    assert err < 2e-4 * max(1.0, float(np.abs(want).max()))


def test_model_in_a_validation_loop(dev, oracle):
    """The trainer's validate_step / forward_pass pattern (train.py:159-222 of the reference:
    eval mode, no_grad, autocast, model(x), a criterion on the logits, thresholded
    precision / recall) works with the HIP-backed module as "self.model"."""
    model, sd = make_model(dev, out_channels=1, seed=5)
    x = normalized_input(oracle, (32, 32, 32), seed=75, n=3)
    y = (torch.rand(3, 1, 32, 32, 32) > 0.7).float()
    criterion = torch.nn.BCEWithLogitsLoss()
    model.eval()
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        hat_y = model(x.to("cuda", dtype=torch.float))
        loss = criterion(hat_y, y.to("cuda", dtype=torch.float))
    want = oracle.unet_forward(x, oracle.OracleModel(sd).sd)
    assert hat_y.dtype == torch.float32 and hat_y.shape == want.shape
    assert abs(float(loss) - float(criterion(want, y))) < 1e-5
    # binarised predictions (compute_stats, train.py:246-247) agree except at |logit| ~ 0
    differ = ((hat_y.cpu() > 0) != (want > 0)) & (want.abs() > 1e-4)
    assert not bool(differ.any())


def test_validation_tiling_loop(dev, oracle, golden):
    """ValidateDataset's deterministic tiling (data_handling.py:384-418) feeding the
    trainer's validate_step (train.py:159-198): zero-overlap patch grid -> centres kept
    by is_contained(buffer=64) (checked against the reference's own helpers, golden g8)
    -> 64^3 patches cut around the centres -> batches through the HIP-backed module under
    no_grad, as the DataLoader loop does; logits against the CPU oracle on the same tiles."""
    from aind_exaspim_neuron_segmentation_amd import inference
    from aind_exaspim_neuron_segmentation_amd.utils import img_util

    g = golden("g8_validation_tiling.npz")
    vol_shape = tuple(int(v) for v in g["case2_vol"])       # (330, 300, 270), 64^3 tiles
    ps = tuple(int(v) for v in g["case2_patch"])
    starts = inference.generate_patch_starts((1, 1) + vol_shape, ps, (0, 0, 0))
    centers = [tuple(v + s // 2 for v, s in zip(st, ps)) for st in starts]
    centers = [c for c in centers if img_util.is_contained(c, vol_shape, buffer=64)]
    np.testing.assert_array_equal(np.array(centers), g["case2_centers_kept"])
    img = oracle.normalize(np.minimum(synthetic.synth_volume(vol_shape, seed=77), 300), percentiles=(1, 99.5))
    tiles = np.stack([img[tuple(slice(c - p // 2, c + p // 2) for c, p in zip(ctr, ps))]
                      for ctr in centers[:6]])[:, None].astype(np.float32)
    model, sd = make_model(dev, out_channels=3, seed=6)
    model.eval()
    outs = []
    with torch.no_grad():
        for i in range(0, len(tiles), 4):                   # DataLoader batches of 4
            outs.append(model(torch.from_numpy(tiles[i:i + 4]).to("cuda", dtype=torch.float)).cpu())
    got = torch.cat(outs).numpy()
    want = oracle.unet_forward(torch.from_numpy(tiles), oracle.OracleModel(sd).sd).numpy()
    err = np.abs(got - want).max()
    print(f"validation tiling loop, {len(tiles)} tiles of {ps}: max|diff| = {err:.3e}")
    assert err < 5e-5


def test_unet_rejects_bad_inputs(dev):
    model, _ = make_model(dev)
    with pytest.raises(RuntimeError, match="Sizes of tensors must match"):
        model(torch.zeros(1, 1, 24, 32, 32, device=dev))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(1, 1, 32, 32, 32))
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model(torch.zeros(1, 1, 32, 32, 32, device=dev))


def test_engine_repacks_after_load_state_dict(dev, oracle):
    model, _ = make_model(dev, seed=1)
    x = normalized_input(oracle, (16, 16, 16), seed=5).to(dev)
    a = model(x).cpu().numpy()
    sd2 = synthetic.synth_state_dict(3, 1, seed=9)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd2.items()})
    b = model(x).cpu().numpy()
    want = oracle.unet_forward(x.cpu(), oracle.OracleModel(sd2).sd).numpy()
    assert np.abs(a - b).max() > 1e-3
    assert np.abs(b - want).max() < 5e-5


# ---------------------------------------------------------- pre-processing ---
def _volumes():
    vol = synthetic.synth_volume((40, 48, 56), seed=3)
    return {
        "u16": vol,
        "u16_sparse": np.where(vol > 1990, vol * 20, vol // 50).astype(np.uint16),
        "f32": (vol.astype(np.float32) * 0.37 - 50.0),
        "u8": (vol % 251).astype(np.uint8),
        "i16": (vol.astype(np.int32) - 1000).astype(np.int16),
        "const": np.full((8, 8, 8), 7, dtype=np.uint16),
    }


@pytest.mark.parametrize("name", list(_volumes()))
@pytest.mark.parametrize("clip,pct", [(1000, (1, 99.9)), (None, (0.5, 75.25)), (300, (0, 100))])
def test_percentiles_bit_exact(dev, name, clip, pct):
    from aind_exaspim_neuron_segmentation_amd import inference

    arr = _volumes()[name]
    vol = inference.DeviceVolume.from_array(arr, dev)
    if clip is not None and arr.dtype == np.uint8 and clip > 255:
        # numpy refuses the clip (inference.py:79 would raise); so must we
        with pytest.raises(OverflowError):
            np.minimum(arr, clip)
        with pytest.raises(OverflowError):
            inference.volume_percentiles(vol, clip, pct)
        return
    ref = np.minimum(arr, clip) if clip is not None else arr
    want = np.percentile(ref, pct)
    mn, mx = inference.volume_percentiles(vol, clip, pct)
    assert (mn, mx) == (want[0], want[1])


@pytest.mark.parametrize("name", ["u16", "f32", "i16", "u8"])
def test_gather_bit_exact(dev, oracle, name):
    from aind_exaspim_neuron_segmentation_amd import inference

    arr = _volumes()[name]  # (40, 48, 56)
    patch, overlap = (32, 32, 48), (8, 4, 40)
    clip = 200 if arr.dtype == np.uint8 else 1000
    clipped = np.minimum(arr, clip)
    mn, mx = np.percentile(clipped, (1, 99.9))
    img = oracle.normalize(clipped)[None, None]
    starts = list(oracle.generate_patch_starts(img.shape, patch, overlap))
    assert len(starts) > 4
    want = oracle.get_batch_inputs(img, starts, patch).numpy()
    vol = inference.DeviceVolume.from_array(arr, dev)
    sdev = torch.tensor(starts, dtype=torch.int32, device=dev)
    got = inference._get_batch_inputs(vol, sdev, patch, dev, clip=clip, mn=mn, mx=mx)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_gather_multi_reflection_and_singleton(dev, oracle):
    from aind_exaspim_neuron_segmentation_amd import inference

    arr = synthetic.synth_volume((33, 17, 1), seed=8)
    patch = (96, 32, 4)
    img = arr.astype(np.float64)[None, None]
    want = oracle.get_batch_inputs(img, [(0, 0, 0)], patch).numpy()
    vol = inference.DeviceVolume.from_array(arr, dev)
    sdev = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    # mn = 0 and denom = 4096 keep every voxel value (< 2000) distinct and exact
    got = inference._get_batch_inputs(vol, sdev, patch, dev, clip=None, mn=0.0, mx=4096.0 - 1e-8)
    np.testing.assert_array_equal(got.cpu().numpy(), (want / 4096.0).astype(np.float32))


# --------------------------------------------------------- post-processing ---
@pytest.mark.parametrize("trim,channels", [(4, 3), (0, 1), (2, 2)])
def test_stitch_bit_exact(dev, trim, channels):
    from aind_exaspim_neuron_segmentation_amd import inference

    shape, patch, overlap = (56, 40, 48), (32, 32, 32), (8, 8, 8)
    plan = inference.SlidingWindow(shape, patch, overlap, trim)
    starts = plan.starts()
    rng = np.random.default_rng(0)
    preds = rng.random((len(starts), channels) + patch, dtype=np.float32)
    accum = np.zeros((channels,) + shape, np.float32)
    wgt = np.zeros(shape, np.float16)
    o = [p - 2 * trim for p in patch]
    for p, s in zip(preds, starts):
        s0 = [si + trim for si in s]
        e = [min(a + b, d) for a, b, d in zip(s0, o, shape)]
        sl = tuple(slice(a, b) for a, b in zip(s0, e))
        ps = tuple(slice(trim, trim + b - a) for a, b in zip(s0, e))
        accum[(slice(None),) + sl] += p[(slice(None),) + ps]
        wgt[sl] += 1
    np.divide(accum, wgt, out=accum, where=wgt != 0)

    block = inference._native.Block.make(shape)
    acc_dev = torch.zeros((channels,) + shape, dtype=torch.float32, device=dev)
    sdev = torch.tensor(starts, dtype=torch.int32, device=dev)
    pdev = torch.tensor(preds, device=dev)
    for i in range(0, len(starts), 5):
        inference.stitch_accumulate(pdev[i:i + 5].contiguous(), sdev[i:i + 5], plan, acc_dev, block)
    inference.stitch_finalize(acc_dev, plan, block)
    np.testing.assert_array_equal(acc_dev.cpu().numpy(), accum)


# --------------------------------------------------------------- end to end ---
def test_predict_fp32_vs_reference_golden_and_oracle(dev, oracle, golden):
    from aind_exaspim_neuron_segmentation_amd import inference

    g = golden("g5_fullwidth_small.npz")
    vol = synthetic.synth_volume((72, 40, 56), seed=11)
    model, sd = make_model(dev)
    kw = dict(batch_size=4, patch_shape=(32, 32, 32), overlap=(8, 8, 8), trim=4)
    got = inference.predict(vol, model, verbose=False, **kw)
    assert got.dtype == np.float32 and got.shape == (3, 72, 40, 56)
    err_ref = np.abs(got[:, ::2, ::2, ::2] - g["pred"]).max()
    want = oracle.predict(vol, oracle.OracleModel(sd), **kw)
    err = np.abs(got - want).max()
    print(f"predict fp32: vs reference golden {err_ref:.3e}, vs oracle {err:.3e}")
    assert err_ref < 5e-6 and err < 5e-6
    np.testing.assert_array_equal(got == 0, want == 0)  # uncovered border stays exactly 0

    model1, sd1 = make_model(dev, out_channels=1, seed=4)
    kw1 = dict(batch_size=5, patch_shape=(32, 32, 32), overlap=(16, 16, 16), trim=2)
    got1 = inference.predict(vol, model1, affinity_mode=False, verbose=False, **kw1)
    assert got1.shape == (72, 40, 56)
    assert np.abs(got1[::2, ::2, ::2] - g["pred_fg"]).max() < 5e-6


def test_predict_default_config_160_vs_reference_golden(dev, golden):
    from aind_exaspim_neuron_segmentation_amd import inference

    g = golden("g6_default_160.npz")
    vol = synthetic.synth_volume((160, 160, 160), seed=0)
    model, _ = make_model(dev)
    got = inference.predict(vol, model, batch_size=8, verbose=False)
    err = np.abs(got[:, ::5, ::5, ::5] - g["pred_sub"]).max()
    print(f"predict 160^3 defaults vs reference: {err:.3e}")
    assert err < 5e-6
    assert np.abs(got[:, 80, 81, :] - g["pred_line"]).max() < 5e-6
    zero = (got == 0).all(axis=0)
    assert abs(zero.mean() - float(g["zero_fraction"])) < 1e-12
    np.testing.assert_array_equal(zero.all(axis=(1, 2)), g["zero_z"])
    # determinism: the stitch has no atomics
    again = inference.predict(vol, model, batch_size=8, verbose=False)
    np.testing.assert_array_equal(got, again)


def test_predict_input_variants(dev, oracle):
    from aind_exaspim_neuron_segmentation_amd import inference

    model, sd = make_model(dev)
    vol = synthetic.synth_volume((40, 48, 40), seed=13)
    kw = dict(batch_size=2, patch_shape=(32, 32, 32), overlap=(8, 8, 8), trim=0,
              brightness_clip=400, normalization_percentiles=(5, 95))
    volf = (vol.astype(np.float32) * 0.5)[None, None]
    want = oracle.predict(volf, oracle.OracleModel(sd), **kw)
    got = inference.predict(volf, model, verbose=False, **kw)
    assert np.abs(got - want).max() < 5e-6
    # volume smaller than the overlap on one axis -> no patches -> zeros
    tiny = synthetic.synth_volume((8, 48, 40), seed=1)
    out = inference.predict(tiny, model, verbose=False, **kw)
    assert out.shape == (3, 8, 48, 40) and not out.any()
    with pytest.raises(RuntimeError, match="multiples of 16"):
        inference.predict(vol, model, patch_shape=(24, 32, 32), overlap=(8, 8, 8), verbose=False)


def test_predict_streams_do_not_change_the_result(dev):
    """predict(n_streams=k): batches in flight on k HIP streams, stitched in batch order."""
    from aind_exaspim_neuron_segmentation_amd import inference

    model, _ = make_model(dev, compute_dtype="bf16")
    vol = synthetic.synth_volume((72, 88, 104), seed=21)
    kw = dict(batch_size=3, patch_shape=(32, 32, 32), overlap=(8, 8, 8), trim=4, verbose=False)
    one = inference.predict(vol, model, **kw)
    for k in (2, 3):
        assert np.array_equal(inference.predict(vol, model, n_streams=k, **kw), one)


def test_synth_volume_matches_numpy(dev):
    from aind_exaspim_neuron_segmentation_amd import _native

    shape, origin, gshape = (5, 7, 9), (3, 2, 1), (16, 12, 10)
    t = torch.empty(shape, dtype=torch.int16, device=dev)
    blk = _native.Block.make(shape, origin, gshape)
    _native.check(_native.lib().exaspim_synth_volume_u16(t.data_ptr(), blk, 5, None), "synth")
    want = synthetic.synth_volume(shape, seed=5, origin=origin, global_shape=gshape)
    np.testing.assert_array_equal(t.cpu().numpy().view(np.uint16), want)


# ------------------------------------------------ full-size (BASELINE configs[1]) ---
def _periodic_volume(edge, seed=17):
    """Volume whose 64^3 cells are identical: with stride 64 every patch that is
    not reflect-padded sees the same input, so the stitched output is periodic."""
    cell = synthetic.synth_volume((64, 64, 64), seed=seed)
    cell[cell < 60] = 0  # 3 % exact zeros: the 1st percentile is 0 for every crop
    reps = -(-edge // 64)
    return np.tile(cell, (reps, reps, reps))[:edge, :edge, :edge].copy()


def test_full_size_512_periodic_property_and_oracle(dev, oracle):
    """512^3 (BASELINE configs[1]) through a size-independent property: a
    64-periodic input gives a 64-periodic output away from the borders, and that
    output equals the CPU oracle's on a 224^3 crop of the same periodic input."""
    from aind_exaspim_neuron_segmentation_amd import inference

    model, sd = make_model(dev)
    big = _periodic_volume(512)
    small = _periodic_volume(224)
    # same percentile pair on both sizes (the value distribution is the same)
    assert tuple(np.percentile(np.minimum(big, 1000), (1, 99.9))) == tuple(
        np.percentile(np.minimum(small, 1000), (1, 99.9))
    )
    got = inference.predict(big, model, batch_size=8, verbose=False)
    assert got.shape == (3, 512, 512, 512)
    # 1. periodicity of the region covered only by unpadded patches: [72, 456)
    a = got[:, 72:392, 72:392, 72:392]
    assert np.abs(a[:, :256] - a[:, 64:320]).max() < 1e-6
    assert np.abs(a[:, :, :256] - a[:, :, 64:320]).max() < 1e-6
    assert np.abs(a[:, :, :, :256] - a[:, :, :, 64:320]).max() < 1e-6
    # 2. borders: first 8 voxels are never covered; 512 = 448 + 64 is covered to the end
    assert not got[:, :8].any() and not got[:, :, :8].any() and not got[:, :, :, :8].any()
    assert got[:, 511, 100, 100].all()
    # 3. against the oracle on the 224^3 crop (27 patches), mapped through the period
    want = oracle.predict(small, oracle.OracleModel(sd), batch_size=9)
    idx = np.arange(8, 456)
    src = np.where(idx < 136, idx, 72 + (idx - 72) % 64)
    sub = np.ix_(np.arange(3), idx[::7], idx[::5], idx)
    ref = np.ix_(np.arange(3), src[::7], src[::5], src)
    err = np.abs(got[sub] - want[ref]).max()
    print(f"512^3 periodic vs oracle(224^3): max|diff| = {err:.3e}")
    assert err < 5e-6


def test_full_size_1024_bf16_periodic_property(dev):
    """1024^3, bf16, batch 16 (BASELINE configs[2], the benchmark's workload) through the same
    size-independent property, checked on the device: a 64-periodic input gives an output that
    is bit-for-bit 64-periodic wherever only unpadded patches contribute (every such patch
    sees the same input and the kernels are deterministic), borders behave as in the
    reference, and the interior equals the 512^3 result of the same model."""
    from aind_exaspim_neuron_segmentation_amd import inference

    model, _ = make_model(dev, compute_dtype="bf16")
    big = _periodic_volume(1024)
    got = inference.predict(big, model, batch_size=16, verbose=False, return_device_tensor=True)
    assert tuple(got.shape) == (3, 1024, 1024, 1024) and got.dtype == torch.float32
    a = got[:, 72:904, 72:904, 72:904]          # covered by unpadded patches only ([72, 968))
    assert torch.equal(a[:, :768], a[:, 64:832])
    assert torch.equal(a[:, :, :768], a[:, :, 64:832])
    assert torch.equal(a[:, :, :, :768], a[:, :, :, 64:832])
    assert not bool(got[:, :8].any()) and not bool(got[:, :, :8].any()) and not bool(got[:, :, :, :8].any())
    assert bool(got[:, 1023, 500, 500].all())
    assert bool(torch.isfinite(got[:, ::37, ::41, ::43]).all())
    cell = got[:, 136:200, 136:200, 136:200].clone()
    del got, a
    small = inference.predict(_periodic_volume(512), model, batch_size=16, verbose=False,
                              return_device_tensor=True)
    assert torch.equal(small[:, 136:200, 136:200, 136:200], cell)


def test_half_width_model_channel_padding(dev, oracle):
    """width_multiplier = 0.5 (16..256 channels): every level is padded to 32
    channels inside the engine; results must not change."""
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(3, 0.5, seed=6)
    model = UNet3D(output_channels=3, width_multiplier=0.5)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model.to(dev).eval()
    x = normalized_input(oracle, (32, 32, 48), seed=50, n=2)
    want = oracle.unet_forward(x, oracle.OracleModel(sd).sd).numpy()
    got = model(x.to(dev)).cpu().numpy()
    assert np.abs(got - want).max() < 5e-5


@pytest.mark.parametrize("cdt,tol", [("fp16", 1e-3), ("bf16", 4e-3)])
def test_predict_16bit_default_config_vs_reference_golden(dev, golden, cdt, tol):
    """Reference defaults on 160^3 in the 16-bit modes against the reference's own
    output: fp16 storage (the mode bench.py runs) meets north_star's 1e-3 on the
    maximum; bf16 (8 significant bits) is held to 4e-3."""
    from aind_exaspim_neuron_segmentation_amd import inference

    g = golden("g6_default_160.npz")
    vol = synthetic.synth_volume((160, 160, 160), seed=0)
    model, _ = make_model(dev, compute_dtype=cdt)
    got = inference.predict(vol, model, batch_size=8, verbose=False)
    err = np.abs(got[:, ::5, ::5, ::5] - g["pred_sub"])
    print(f"predict 160^3 {cdt} vs reference: max {err.max():.3e} mean {err.mean():.3e} "
          f"p99.9 {np.quantile(err, 0.999):.3e}")
    assert err.max() < tol
    zero = (got == 0).all(axis=0)
    np.testing.assert_array_equal(zero.all(axis=(1, 2)), g["zero_z"])


@pytest.mark.parametrize("name,clip", [("u8", 200), ("i16", 500), ("f32", 123.5), ("u16_sparse", 1000)])
def test_predict_voxel_dtypes_vs_oracle(dev, oracle, name, clip):
    """End to end for every voxel dtype the ABI takes (uint8, int16, float32, uint16)."""
    from aind_exaspim_neuron_segmentation_amd import inference

    vol = _volumes()[name]  # (40, 48, 56)
    model, sd = make_model(dev)
    kw = dict(batch_size=4, patch_shape=(32, 32, 32), overlap=(16, 8, 8), trim=4,
              brightness_clip=clip, normalization_percentiles=(2, 98.5))
    want = oracle.predict(vol, oracle.OracleModel(sd), **kw)
    got = inference.predict(vol, model, verbose=False, **kw)
    err = np.abs(got - want).max()
    print(f"predict {name}: max|diff| = {err:.3e}")
    assert err < 5e-6
    np.testing.assert_array_equal(got == 0, want == 0)


@pytest.mark.parametrize("name,clip", [("i32", 1000), ("u32", 700), ("i64", 1000), ("u64", 900), ("f64", 123.5),
                                       ("i8", 100), ("u16_fractional_clip", 1000.5), ("u8_fractional_clip", 200.25),
                                       ("i32_fractional_clip", 800.5),
                                       ("u16_typed_clip", np.int64(1000)), ("i16_wide_range", np.int32(40000)),
                                       ("i32", np.int64(650))])
def test_predict_takes_the_dtypes_the_reference_takes(dev, oracle, name, clip):
    """inference.py:79-80 runs on any numeric array: wider integers and float64 travel to
    the device as float32 when the array shows that float32 holds every value (as float64
    otherwise, next test), int8 as int16, and a clip that
    makes np.minimum promote an integer image to float64 is evaluated the same way
    (voxels above it take the clip's own, fractional, value)."""
    from aind_exaspim_neuron_segmentation_amd import inference

    base = _volumes()["u16"]  # (40, 48, 56), values 0..1999
    vol = {
        "i32": base.astype(np.int32) - 300,
        "u32": base.astype(np.uint32) * 3,
        "i64": base.astype(np.int64) * 7 - 2000,
        "u64": base.astype(np.uint64),
        "f64": base.astype(np.float64) * 0.25 - 11.5,
        "i8": (base % 251).astype(np.int16).astype(np.int8),
        "u16_fractional_clip": base,
        "u8_fractional_clip": (base % 251).astype(np.uint8),
        "i32_fractional_clip": base.astype(np.int32) - 300,
        # a typed integer clip widens the image in np.minimum: the same voxels, wider arithmetic in
        # np.percentile (an int16 difference of order statistics 60 000 apart would wrap)
        "u16_typed_clip": base,
        "i16_wide_range": (base.astype(np.int32) * 32 - 32000).astype(np.int16),
    }[name]
    model, sd = make_model(dev)
    kw = dict(batch_size=4, patch_shape=(32, 32, 32), overlap=(16, 8, 8), trim=4,
              brightness_clip=clip, normalization_percentiles=(2, 98.5))
    want = oracle.predict(vol, oracle.OracleModel(sd), **kw)
    got = inference.predict(vol, model, verbose=False, **kw)
    err = np.abs(got - want).max()
    print(f"predict {name}: max|diff| = {err:.3e}")
    assert err < 5e-6
    np.testing.assert_array_equal(got == 0, want == 0)
    # percentiles are numpy's, bit for bit
    dv = inference.DeviceVolume.from_array(vol, dev)
    mn, mx = inference.volume_percentiles(dv, clip, (2, 98.5))
    ref = np.percentile(np.minimum(vol, clip), (2, 98.5))
    assert (mn, mx) == (ref[0], ref[1])


@pytest.mark.parametrize("name,clip", [
    ("f64_fractions", 1000), ("f64_fractions", 123.456789), ("f64_fractions", None),
    ("i64_beyond_float32", 1 << 41), ("u32_beyond_float32", 4_000_000_001), ("i32_irrational_clip", 0.1 + 900),
    ("f64_negative", 3.0),
])
def test_predict_takes_what_float32_cannot_carry(dev, oracle, name, clip):
    """The reference takes ANY numeric array and works in float64 (inference.py:79-80,
    img_util.py:526-531). Values float32 cannot hold -- fractions of a float64 image, integers
    beyond 2^24, a clip that is no float32 number -- travel to the device as float64: four-pass
    histogram on a 64-bit key (exaspim_histogram_wide), float64 gather. Percentiles equal numpy's
    bit for bit, predict() the oracle's."""
    from aind_exaspim_neuron_segmentation_amd import inference

    base = _volumes()["u16"].astype(np.float64)  # (40, 48, 56), values 0..1999
    rng = np.random.default_rng(5)
    vol = {
        "f64_fractions": base + rng.random(base.shape),                       # 52-bit fractions
        "i64_beyond_float32": base.astype(np.int64) * ((1 << 30) + 1) + 7,    # up to 2^41, odd
        "u32_beyond_float32": (base.astype(np.uint32) * 2_100_003 + 17),      # up to 4.2e9
        "i32_irrational_clip": base.astype(np.int32) - 300,
        "f64_negative": rng.normal(0.0, 2.0, base.shape),
    }[name]
    model, sd = make_model(dev)
    kw = dict(batch_size=4, patch_shape=(32, 32, 32), overlap=(16, 8, 8), trim=4,
              brightness_clip=clip, normalization_percentiles=(2, 98.5))
    dv = inference.DeviceVolume.from_array(vol, dev, clip=clip)
    assert dv.storage_dtype == np.float64 and dv.tensor.dtype == torch.float64
    mn, mx = inference.volume_percentiles(dv, clip, (2, 98.5))
    ref = np.percentile(np.minimum(vol, clip) if clip is not None else vol, (2, 98.5))
    assert (mn, mx) == (ref[0], ref[1])
    want = oracle.predict(vol, oracle.OracleModel(sd), **kw) if clip is not None else None
    got = inference.predict(vol, model, verbose=False, **kw)
    if want is None:        # the oracle (like the reference) always clips: compare through a clip above every voxel
        want = oracle.predict(vol, oracle.OracleModel(sd), **dict(kw, brightness_clip=1e300))
    err = np.abs(got - want).max()
    print(f"predict {name}, clip {clip}: max|diff| = {err:.3e}")
    assert err < 5e-6
    np.testing.assert_array_equal(got == 0, want == 0)
    # the device-resident route and a chunked source (no knowledge of the values: float64 carrier)
    t = inference.predict(vol, model, verbose=False, return_device_tensor=True, **kw)
    np.testing.assert_array_equal(t.cpu().numpy(), got)
    got2 = inference.predict_streaming(lambda z0, z1: vol[z0:z1], model, verbose=False, shape=vol.shape,
                                       dtype=vol.dtype, **kw)
    np.testing.assert_array_equal(got2, got)


def test_predict_rejects_what_no_float_can_carry(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    model, _ = make_model(dev)
    vol = _volumes()["u16"]
    kw = dict(patch_shape=(32, 32, 32), overlap=(8, 8, 8), trim=4, verbose=False)
    with pytest.raises(TypeError, match="not exactly representable in float64"):
        inference.predict(vol.astype(np.int64) + ((1 << 60) + 1), model, **kw)
    with pytest.raises(TypeError, match="not supported"):
        inference.predict(vol.astype(np.complex64), model, **kw)
    with pytest.raises(OverflowError):          # numpy's own refusal (inference.py:79)
        inference.predict((vol % 251).astype(np.uint8), model, brightness_clip=1000, **kw)
    # a clip below every voxel an unsigned image can hold has no histogram bin to stand in: refused in
    # Python, and again at the C ABI (which must never index a bin below zero)
    with pytest.raises(NotImplementedError, match="below every"):
        inference.predict(vol, model, brightness_clip=-3.5, **kw)
    from aind_exaspim_neuron_segmentation_amd import _native
    t = torch.from_numpy(vol.view(np.int16)).to(dev)
    hist = torch.zeros(65536, dtype=torch.int64, device=dev)
    rc = _native.lib().exaspim_histogram(t.data_ptr(), _native.VOX_U16, t.numel(), -3.5, 1, 0, 0, hist.data_ptr(), None)
    assert rc == -1 and "below every voxel" in _native.last_error()
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("wm,shape,n", [(1, (96, 96, 96), 2), (1, (48, 64, 80), 3), (0.5, (32, 48, 64), 2),
                                        (2, (16, 32, 48), 1), (0.25, (96, 32, 16), 5)])
def test_fused_max_pool_equals_the_separate_launch(dev, oracle, dtype, wm, shape, n):
    """The last convolution of every encoder level writes the level's MaxPool3d(2)
    (unet3d.py:194-196) from its epilogue (z-column kernel: wave-local; t14 kernel: the
    tile's output groups parked in LDS, 16-bit modes). The engine option EXASPIM_OPT_SEPARATE_POOL
    (exaspim_unet_set_options) runs the stand-alone max-pool launches instead: the logits must be the same bits
    -- a maximum of stored values either way -- over the tile shapes of all pyramid levels
    (96/48/24/12, 80/40/20/10, 64/32/16/8 ... wide), widths and dtypes."""
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(3, wm, seed=23)
    model = UNet3D(output_channels=3, width_multiplier=wm, compute_dtype=dtype)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = model.to(dev).eval()
    x = normalized_input(oracle, shape, seed=31, n=n).to(dev)
    from aind_exaspim_neuron_segmentation_amd import _native

    fused = model(x).cpu().numpy()
    model.engine_options = _native.OPT_SEPARATE_POOL
    separate = model(x).cpu().numpy()
    model.engine_options = 0
    assert np.array_equal(model(x).cpu().numpy(), fused)
    assert np.isfinite(fused).all()
    assert np.array_equal(fused, separate)


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("wm,shape,n,trim", [(1, (96, 96, 96), 2, 8), (1, (96, 96, 96), 1, 0), (1, (48, 64, 80), 3, 4),
                                             (0.5, (32, 48, 64), 2, 6), (2, (16, 32, 48), 1, 2), (1, (96, 96, 96), 1, 7),
                                             (0.25, (96, 32, 16), 5, 0), (1, (64, 80, 96), 2, 6),
                                             (0.5, (96, 32, 128), 1, 8)])
def test_pipelined_upsampling_equals_the_plain_kernel(dev, oracle, dtype, wm, shape, n, trim):
    """nn.Upsample(x2, trilinear, align_corners=True) (unet3d.py:248-250) runs on a software-pipelined
    kernel whenever the first output plane it has to produce is even (every level of the full forward; the
    trimmed forward's level 0 with an even margin trim - 2): one new source plane per pair of output planes,
    fetched a pair ahead, branch-free range-checked stores. The engine option EXASPIM_OPT_PLAIN_UPSAMPLE
    runs the plain kernel instead: same arithmetic in the same order, so the same bits -- over the pyramid
    levels of several patch shapes (96/48/24/12, 80/40/20/10 ... wide; source depths down to 1 plane, where
    the plain kernel is the only one), widths, dtypes, and odd trims (plain kernel either way).
    The trimmed forward's level 0 (margin >= 4, a whole number of 14- or 12-pair runs, source rows of a
    workgroup within 512 pieces: 96^3 / trim 8, 32x48x64 / trim 6, 64x80x96 / trim 6) goes one step further
    and shares a workgroup's source rows through LDS (upsample2_strip_kernel); EXASPIM_OPT_UPSAMPLE_PER_THREAD
    keeps the per-thread pipeline. All three must produce the same bits."""
    from aind_exaspim_neuron_segmentation_amd import _native
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(3, wm, seed=29)
    model = UNet3D(output_channels=3, width_multiplier=wm, compute_dtype=dtype)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = model.to(dev).eval()
    x = normalized_input(oracle, shape, seed=37, n=n).to(dev)
    inner = (Ellipsis,) + ((slice(trim, -trim),) * 3 if trim else (slice(None),) * 3)
    piped = model.run(x, apply_sigmoid=True, trim=trim)[inner].cpu().numpy()
    model.engine_options = _native.OPT_UPSAMPLE_PER_THREAD
    per_thread = model.run(x, apply_sigmoid=True, trim=trim)[inner].cpu().numpy()
    model.engine_options = _native.OPT_PLAIN_UPSAMPLE
    plain = model.run(x, apply_sigmoid=True, trim=trim)[inner].cpu().numpy()
    model.engine_options = 0
    assert np.isfinite(piped).all()
    assert np.array_equal(piped, plain)
    assert np.array_equal(per_thread, plain)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("wm,shape,n", [(1, (96, 96, 96), 3), (1, (16, 32, 64), 5), (2, (32, 48, 128), 2), (0.5, (48, 16, 32), 7),
                                        (1, (32, 32, 160), 1), (1, (32, 16, 48), 2)])
def test_row_strip_first_convolution_equals_the_per_group_kernel(dev, oracle, dtype, wm, shape, n):
    """inc.0 of the 16-bit modes (Conv3d(1 -> C0), unet3d.py:64,143-145) runs on row strips -- four rows x the
    whole width per workgroup, the taps' input words staged once in LDS -- whenever the width is a multiple of
    32 up to 128; the engine option EXASPIM_OPT_FIRST_PER_GROUP keeps the kernel that loads 16 taps per
    32-voxel group. Same operands to the same MFMAs: the logits must be the same bits (widths 32 / 64 / 96 /
    128 = one to four groups per wave, two cout slices, and shapes where the strip kernel does not apply)."""
    from aind_exaspim_neuron_segmentation_amd import _native
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(3, wm, seed=41)
    model = UNet3D(output_channels=3, width_multiplier=wm, compute_dtype=dtype)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = model.to(dev).eval()
    x = normalized_input(oracle, shape, seed=43, n=n).to(dev)
    strips = model(x).cpu().numpy()
    model.engine_options = _native.OPT_FIRST_PER_GROUP
    groups = model(x).cpu().numpy()
    model.engine_options = 0
    assert np.isfinite(strips).all() and np.array_equal(strips, groups)


def _split_words(x, kind):
    """hi | lo << 16 of float32 values, hi = half(x), lo = half(x - float(hi)) (numpy)."""
    if kind == "f16":
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
        return hi.view(np.uint16).astype(np.uint32) | (lo.view(np.uint16).astype(np.uint32) << 16)

    def bf16(v):      # round to nearest even on the upper 16 bits
        u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
        return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)

    hi = bf16(x)
    lo = bf16(x - (hi << 16).astype(np.uint32).view(np.float32))
    return hi | (lo << 16)


@pytest.mark.parametrize("clip", [16383, 16300, 16384, 40000])
def test_gather_table_path_at_its_largest_clips(dev, oracle, clip):
    """The table of the unsigned-integer gather (one normalised value per voxel value up to the clip) and
    its row map share the 64 KiB of dynamic LDS a launch gets: clips near 16 383 take the generic path once
    the two no longer fit -- plain and zero-bordered split layouts, bit for bit against the oracle."""
    from aind_exaspim_neuron_segmentation_amd import _native, inference

    arr = (synthetic.synth_volume((40, 48, 56), seed=11).astype(np.uint32) * 23 % 50000).astype(np.uint16)
    patch, overlap = (32, 32, 48), (8, 4, 40)
    clipped = np.minimum(arr, clip)
    mn, mx = np.percentile(clipped, (1, 99.9))
    img = oracle.normalize(clipped)[None, None]
    starts = list(oracle.generate_patch_starts(img.shape, patch, overlap))
    want = oracle.get_batch_inputs(img, starts, patch).numpy()
    vol = inference.DeviceVolume.from_array(arr, dev)
    sdev = torch.tensor(starts, dtype=torch.int32, device=dev)
    got = inference._get_batch_inputs(vol, sdev, patch, dev, clip=np.uint16(clip), mn=mn, mx=mx)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    padded = inference._get_batch_inputs(vol, sdev, patch, dev, clip=np.uint16(clip), mn=mn, mx=mx,
                                         layout=_native.IN_PADDED_F32).cpu().numpy()
    padded = padded.reshape((len(starts),) + tuple(p + 2 for p in patch))
    np.testing.assert_array_equal(padded[:, 1:-1, 1:-1, 1:-1], want[:, 0])
    assert not padded[:, 0].any() and not padded[:, :, -1].any() and not padded[..., 0].any()


@pytest.mark.parametrize("vox,clip", [(np.uint16, 1000), (np.float32, None), (np.int16, 700.5), (np.uint8, 200)])
def test_gather_writes_the_first_convolutions_operand_layout(dev, vox, clip):
    """exaspim_gather_patches_as: the zero-bordered float32 copy and the hi | lo << 16 split
    copies (IEEE half, bfloat16) of a batch equal what numpy makes of the float32 batch the
    reference-shaped gather returns -- table path, generic path, reflected and ragged patches."""
    from aind_exaspim_neuron_segmentation_amd import _native, inference

    rng = np.random.default_rng(3)
    vol = (rng.random((41, 37, 52)) * 1500).astype(vox)
    volume = inference.DeviceVolume.from_array(vol, dev)
    starts = torch.tensor([[0, 0, 0], [16, 8, 24], [32, 24, 40], [9, 5, 20]], dtype=torch.int32, device=dev)
    patch = (32, 16, 48)
    c, _ = inference._effective_clip(volume.np_dtype, clip, volume.storage_dtype)
    kw = dict(clip=c, mn=3.0, mx=977.0)
    plain = inference._get_batch_inputs(volume, starts, patch, dev, **kw).cpu().numpy()[:, 0]
    padded = np.zeros((4, 34, 18, 50), np.float32)
    padded[:, 1:-1, 1:-1, 1:-1] = plain
    got = inference._get_batch_inputs(volume, starts, patch, dev, layout=_native.IN_PADDED_F32, **kw)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), padded.view(np.uint32))
    for layout, kind in ((_native.IN_PADDED_SPLIT_F16, "f16"), (_native.IN_PADDED_SPLIT_BF16, "bf16")):
        got = inference._get_batch_inputs(volume, starts, patch, dev, layout=layout, **kw)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), _split_words(padded, kind)), kind


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_prepared_gather_path_does_not_change_a_bit(dev, dtype, monkeypatch):
    """predict() lets the gather kernel write the first convolution's operand layout
    (exaspim_unet_forward_prepared); inference.PLAIN_GATHER goes through the float32 batch
    and the engine's own padding pass, like model(inputs) does. Same bits."""
    from aind_exaspim_neuron_segmentation_amd import inference

    model, _ = make_model(dev, seed=9, compute_dtype=dtype)
    vol = synthetic.synth_volume((72, 88, 104), seed=5)
    kw = dict(batch_size=5, patch_shape=(32, 48, 32), overlap=(8, 8, 8), trim=4, verbose=False)
    fused = inference.predict(vol, model, **kw)
    monkeypatch.setattr(inference, "PLAIN_GATHER", True)
    plain = inference.predict(vol, model, **kw)
    monkeypatch.setattr(inference, "PLAIN_GATHER", False)
    assert fused.any() and np.array_equal(fused, plain)
