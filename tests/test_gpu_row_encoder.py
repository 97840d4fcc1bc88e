"""Row mode of the first level (exaspim_unet_forward_prepared_row): the patches of a batch that is one
row along x share columns, inc.3 computes each of them once and the thin-tile and column max-pool
launches redo the two outermost x of every patch face that borders a neighbour. The result must be
the bits of the per-patch path (EXASPIM_OPT_PER_PATCH_ENCODER), for every geometry the engine takes
the row path on and every one it must refuse."""
import numpy as np
import pytest
import torch

import layer_ref as R
from aind_exaspim_neuron_segmentation_amd import _native, inference
from aind_exaspim_neuron_segmentation_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(dev, dtype):
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(3, 1, seed=41)
    model = UNet3D(output_channels=3, width_multiplier=1, compute_dtype=dtype)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return model.to(dev).eval()


def _run(model, dev, starts, patch, trim, row_stride, vol_shape, seed=5):
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, 1200, size=vol_shape, dtype=np.uint16)
    dvol = inference.DeviceVolume.from_array(vol, dev)
    sdev = torch.tensor(starts, dtype=torch.int32, device=dev).reshape(-1, 3)
    layout = model.input_layout(dev)
    x = inference._get_batch_inputs(dvol, sdev, patch, dev, clip=np.uint16(1000), mn=19.0, mx=1000.0,
                                    layout=layout)
    shape = (len(starts),) + tuple(patch)
    outs = []
    for opt in (0, _native.OPT_PER_PATCH_ENCODER):
        model.engine_options = opt
        outs.append(model.run_prepared(x, shape, apply_sigmoid=True, trim=trim,
                                       row_stride=row_stride).cpu().numpy())
    model.engine_options = 0
    if trim > 0:    # (voxels within trim of a face are not written)
        outs = [o[..., trim:-trim, trim:-trim, trim:-trim] for o in outs]
    return outs


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("trim", [8, 0])
@pytest.mark.parametrize("n", [2, 3, 16])
def test_row_of_96_patches_equals_per_patch(dev, dtype, trim, n):
    model = _model(dev, dtype)
    starts = [(0, 0, 64 * i) for i in range(n)]
    row, per_patch = _run(model, dev, starts, (96, 96, 96), trim, 64, (96, 96, 64 * n + 32))
    assert np.isfinite(row).all()
    assert np.array_equal(row, per_patch)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("trim", [8, 0])
def test_row_of_64_patches_equals_per_patch(dev, dtype, trim):
    model = _model(dev, dtype)
    starts = [(0, 16, 32 * i) for i in range(5)]
    row, per_patch = _run(model, dev, starts, (64, 64, 64), trim, 32, (64, 80, 32 * 5 + 32))
    assert np.array_equal(row, per_patch)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_geometries_that_fall_back(dev, dtype):
    model = _model(dev, dtype)
    # overlap 16: not a multiple of 32, the engine takes the per-patch path
    starts = [(0, 0, 80 * i) for i in range(3)]
    a, b = _run(model, dev, starts, (96, 96, 96), 8, 80, (96, 96, 256))
    assert np.array_equal(a, b)
    # a batch that spans two rows is no row: the caller passes 0
    starts = [(0, 0, 0), (0, 0, 64), (0, 64, 0)]
    assert inference.batch_row_stride(starts, (96, 96, 96), (32, 32, 32)) == 0
    a, b = _run(model, dev, starts, (96, 96, 96), 8, 0, (96, 160, 160))
    assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("batch_size", [5, 4])
def test_predict_equals_per_patch(dev, dtype, batch_size):
    # 2 rows of 5 patches: batch 5 gives full rows, batch 4 rows, mixed batches and a ragged tail
    model = _model(dev, dtype)
    rng = np.random.default_rng(9)
    vol = rng.integers(0, 1200, size=(96, 160, 352), dtype=np.uint16)
    kw = dict(batch_size=batch_size, patch_shape=(96, 96, 96), overlap=(32, 32, 32), trim=8, verbose=False)
    row = inference.predict(vol, model, **kw)
    model.engine_options = _native.OPT_PER_PATCH_ENCODER
    per_patch = inference.predict(vol, model, **kw)
    model.engine_options = 0
    assert np.array_equal(np.asarray(row), np.asarray(per_patch))


# ---- the comparisons above are row mode against per-patch, not per-patch against per-patch ----------------
@pytest.fixture(scope="module")
def probe():
    import __graft_entry__

    __graft_entry__.build()
    return R.load_probe()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_row_cases_take_row_mode(probe, dt):
    """conv_row_mode_ok -- the engine's predicate and the launcher's argument check -- says yes to the
    inc.3 geometry of every case this file calls a row case, and no to the two that fall back."""
    cout = R.plan_conv(probe, [32, 64, 128, 256, 512], 3, dt, 0)[5]   # inc.3 of _model (width multiplier 1)
    ok = lambda n, w, stride: probe.probe_conv_row_mode_ok(R.DTYPES[dt], cout, n, w, stride, 1)   # noqa: E731
    for n in (2, 3, 16):
        assert ok(n, 96, 64) == 1     # test_row_of_96_patches_equals_per_patch
    assert ok(5, 64, 32) == 1         # test_row_of_64_patches_equals_per_patch
    assert ok(5, 96, 64) == 1 and ok(4, 96, 64) == 1   # test_predict_equals_per_patch
    assert ok(4, 64, 32) == 1         # test_ragged_row_equals_per_patch
    assert ok(3, 96, 80) == 0         # test_geometries_that_fall_back: overlap 16 ...
    assert ok(3, 96, 0) == 0          # ... and a batch that is no row


RAGGED = dict(vol=(64, 64, 150), patch=(64, 64, 64), overlap=(32, 32, 32))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_ragged_row_equals_per_patch(dev, dtype):
    # one row of four 64^3 patches at x = 0, 32, 64, 96 over 150 voxels: the last one reflects 10
    starts = [tuple(r) for r in inference._start_ranges(RAGGED["vol"], RAGGED["patch"], RAGGED["overlap"])]
    assert starts == [(0,), (0,), (0, 32, 64, 96)]
    assert inference.batch_row_stride([(0, 0, x) for x in starts[2]], RAGGED["patch"], RAGGED["overlap"]) == 32
    model = _model(dev, dtype)
    rng = np.random.default_rng(13)
    vol = rng.integers(0, 1200, size=RAGGED["vol"], dtype=np.uint16)
    kw = dict(batch_size=4, patch_shape=RAGGED["patch"], overlap=RAGGED["overlap"], trim=8, verbose=False)
    row = inference.predict(vol, model, **kw)
    model.engine_options = _native.OPT_PER_PATCH_ENCODER
    per_patch = inference.predict(vol, model, **kw)
    model.engine_options = 0
    assert np.array_equal(np.asarray(row), np.asarray(per_patch))


def test_start_grid_keeps_every_overlap_inside_the_volume():
    """Row mode computes a column two neighbours share from the first one's operands, which is right only
    where that column holds the volume's own voxels in both: the reference's start grid,
    range(0, dim - overlap, stride), ends with last_start + overlap < dim, so only the last patch of a row
    reaches the reflected padding, beyond every column it shares. (No device needed.)"""
    for patch, overlap in [(96, 32), (64, 32), (128, 64), (160, 64), (80, 32), (32, 8)]:
        for dim in range(overlap + 1, 4 * patch + 3):
            (r,) = inference._start_ranges((dim,), (patch,), (overlap,))
            assert len(r) >= 1 and r[0] == 0
            assert r[-1] + overlap < dim, (patch, overlap, dim)
            # the columns a patch shares with its predecessor, [start, start + overlap), are the volume's own
            assert all(b - a == patch - overlap and b + overlap <= dim for a, b in zip(r, r[1:]))
