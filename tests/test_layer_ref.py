"""
CPU checks of the per-layer test machinery (layer_ref.py): the fragment-order weight decoder
against every convolution of a packed image, the blocked layout, and the checker's power to
reject the kernel defects the per-layer GPU tests exist to catch.
"""

import os

import numpy as np
import pytest
import torch

import layer_ref as R
from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic


@pytest.fixture(scope="module")
def probe():
    if not (os.path.exists(_native.LIB_PATH) and os.path.exists(R.PROBE_PATH)):
        import __graft_entry__

        __graft_entry__.build()
    return R.load_probe()


def _flat_params(sd):
    return np.concatenate(
        [v.reshape(-1).astype(np.float32) for k, v in sd.items() if not k.endswith("num_batches_tracked")])


def _mfma_conv_prefixes(sd):
    """State-dict prefixes of the 17 MFMA convolutions, in plan order (inc.3 .. up4.3)."""
    convs = [k[: -len(".weight")] for k, v in sd.items() if k.endswith(".weight") and v.ndim == 5]
    convs = [c for c in convs if c != "inc.double_conv.0" and not c.startswith("outc")]
    assert len(convs) == 17
    return convs


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("wm,widths", [(0.125, [4, 8, 16, 32, 64]), (0.5, [16, 32, 64, 128, 256])])
def test_decode_every_packed_conv_exactly(probe, lib_for_pack, dt, wm, widths):
    sd = synthetic.synth_state_dict(3, wm, seed=11)
    params = _flat_params(sd)
    ch = _native.channels_array(widths)
    code = R.DTYPES[dt]
    nbytes = lib_for_pack.exaspim_unet_packed_bytes(ch, 3, code)
    packed = np.zeros(nbytes, np.uint8)
    _native.check(lib_for_pack.exaspim_unet_pack_weights(ch, 3, code, params.ctypes.data, params.size,
                                                         packed.ctypes.data, nbytes), "pack")
    for layer, prefix in enumerate(_mfma_conv_prefixes(sd)):
        ca_r, cb_r, ca, cb, co_r, co, w_off, b_off = R.plan_conv(probe, widths, 3, dt, layer)
        w64, b64 = R.fold_bn64(sd, prefix)
        assert w64.shape == (co_r, ca_r + cb_r, 27), (prefix, w64.shape)
        got = R.decode_conv_weights(packed, w_off, ca + cb, co, dt)
        want = np.zeros((co, ca + cb, 27))
        want[:co_r, :ca_r] = R.round_like_plan(w64[:, :ca_r], dt)
        want[:co_r, ca: ca + cb_r] = R.round_like_plan(w64[:, ca_r:], dt)
        np.testing.assert_array_equal(got, want, err_msg=f"{dt} {prefix}")
        bias = packed[b_off: b_off + co * 4].view(np.float32)
        np.testing.assert_array_equal(bias[:co_r], b64.astype(np.float32), err_msg=prefix)
        assert not bias[co_r:].any()


@pytest.fixture(scope="module")
def lib_for_pack(probe):
    return _native.lib()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_blocked_layout_round_trip(dt):
    k = R.kc(dt)
    x = torch.randn(2, 2 * k, 3, 4, 5, dtype=torch.float64)
    t = R.pack_blocked(x, dt)
    assert t.shape == (2, 2, 3, 4, 5, k) and t.dtype == R.STORAGE[dt]
    # voxel (1, :, 2, 3, 4) of chunk 1 is one contiguous 32-byte record
    rec = t[1, 1, 2, 3, 4]
    assert rec.numel() * rec.element_size() == 32
    np.testing.assert_array_equal(rec.to(torch.float64).numpy(), R.quantize(x[1, k:, 2, 3, 4], dt).numpy())
    np.testing.assert_array_equal(R.unpack_blocked(t).numpy(), R.quantize(x, dt).numpy())


def test_quantize_saturates_f16_and_keeps_nan():
    x = torch.tensor([70000.0, -1e9, 65504.0, float("nan"), 1.0 + 2 ** -11, 2.0 ** -25])
    q = R.quantize(x, "f16")
    assert q[0] == 65504 and q[1] == -65504 and q[2] == 65504 and torch.isnan(q[3])
    assert q[4] == 1.0 and q[5] == 0.0   # RNE: ties to even, below half the smallest subnormal


def _uniform_pm(shape, gen):
    """uniform +-[0.5, 1): every product is visible in the sum"""
    mag = 0.5 + 0.5 * torch.rand(shape, generator=gen, dtype=torch.float64)
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).to(torch.float64)
    return mag * sign


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_checker_rejects_kernel_defects(dt):
    gen = torch.Generator().manual_seed(5)
    k = R.kc(dt)
    cin, cout, cout_real = 2 * k, 32, 30
    x = R.quantize(_uniform_pm((1, cin, 4, 6, 8), gen), dt)
    w = R.quantize(_uniform_pm((cout, cin, 27), gen), dt)
    w[cout_real:] = 0
    b = torch.zeros(cout, dtype=torch.float64)
    b[:cout_real] = 4.0 * _uniform_pm((cout_real,), gen)
    acc, s = R.conv_ref(x, w, b)
    assert (acc[:, :cout_real] > 0).any() and (acc[:, :cout_real] < 0).any()
    store = lambda a: R.quantize(R.leaky(a), dt)   # noqa: E731

    # the reference itself passes
    R.check_conv(store(acc), acc, s, cin, dt, cout_real=cout_real)

    def rejected(a):
        with pytest.raises(AssertionError):
            R.check_conv(store(a), acc, s, cin, dt, cout_real=cout_real)

    # one tap x one chunk dropped at one voxel (tap 13 = the centre, chunk 1, voxel (2, 3, 4))
    bad = acc.clone()
    t, c, (z, y, xx) = 13, 1, (2, 3, 4)
    bad[0, :, z, y, xx] -= (w[:, c * k: (c + 1) * k, t] * x[0, c * k: (c + 1) * k, z, y, xx]).sum(1)
    rejected(bad)
    # a tile face shifted by one voxel: plane x = 7 holds plane x = 6's values
    bad = acc.clone()
    bad[..., 7] = acc[..., 6]
    rejected(bad)
    # one channel's bias swapped with another's
    bad = acc.clone()
    bad[:, 3] += b[5] - b[3]
    rejected(bad)
    # one split-K range (chunk 0 of 2) added twice
    x0 = x.clone()
    x0[:, k:] = 0
    part, _ = R.conv_ref(x0, w, torch.zeros(cout, dtype=torch.float64))
    rejected(acc + part)
    # a padded output channel written
    out = store(acc)
    out[0, 31, 0, 0, 0] = 1.0
    with pytest.raises(AssertionError):
        R.check_conv(out, acc, s, cin, dt, cout_real=cout_real)
    # a NaN that should have been finite, and a NaN saturated to a finite value
    out = store(acc)
    out[0, 0, 1, 1, 1] = float("nan")
    with pytest.raises(AssertionError):
        R.check_conv(out, acc, s, cin, dt, cout_real=cout_real)
    nan_acc = acc.clone()
    nan_acc[0, 0, 1, 1, 1] = float("nan")
    with pytest.raises(AssertionError):
        R.check_conv(store(acc), nan_acc, s, cin, dt, cout_real=cout_real)


# (d, h, w, org + ext): interior, touching faces (the grown box is clipped), a thin tile, the whole patch
FOOTPRINTS = [
    (8, 12, 20, (1, 2, 3, 6, 9, 14)),
    (6, 12, 16, (2, 0, 5, 3, 12, 11)),
    (12, 16, 16, (2, 13, 8, 8, 2, 8)),
    (6, 8, 16, (1, 0, 14, 4, 8, 2)),
    (4, 6, 8, (0, 0, 0, 4, 6, 8)),
]


@pytest.mark.parametrize("case", FOOTPRINTS, ids=lambda c: "-".join(map(str, c[3])))
def test_poison_mask_is_the_read_footprint_of_a_region(case):
    """The mask the GPU layer tests poison with (src_poison): in the float64 reference, NaN everywhere
    outside the region grown by one voxel leaves every output of the region as it was, and a NaN in any
    single voxel of the grown box's shell (inside the box, outside the region) reaches the region."""
    d, h, w, region = case
    (oz, oy, ox), (ez, ey, ex) = region[:3], region[3:]
    gen = torch.Generator().manual_seed(sum(region))
    cin, cout = 8, 4
    x = _uniform_pm((2, cin, d, h, w), gen)
    wt = _uniform_pm((cout, cin, 27), gen)
    b = _uniform_pm((cout,), gen)
    inside = (Ellipsis, slice(oz, oz + ez), slice(oy, oy + ey), slice(ox, ox + ex))
    acc, _ = R.conv_ref(x, wt, b)
    box = R.grown_box((d, h, w), region)
    want = torch.zeros((d, h, w), dtype=torch.bool)
    want[max(0, oz - 1): oz + ez + 1, max(0, oy - 1): oy + ey + 1, max(0, ox - 1): ox + ex + 1] = True
    assert torch.equal(box, want)
    xp = R.poison_outside(x, region)
    assert torch.equal(torch.isnan(xp), (~box).expand(2, cin, d, h, w)) and torch.equal(xp[:, :, box], x[:, :, box])
    acc_p, _ = R.conv_ref(xp, wt, b)
    assert not torch.isnan(acc_p[inside]).any()
    assert torch.equal(acc_p[inside], acc[inside])
    # every voxel of the shell is read: one NaN there, in one channel of one patch, changes the region
    shell = box.clone()
    shell[oz: oz + ez, oy: oy + ey, ox: ox + ex] = False
    for z, y, xx in shell.nonzero().tolist():
        one = xp.clone()
        one[1, 3, z, y, xx] = float("nan")
        hit = torch.isnan(R.conv_ref(one[1:], wt, b)[0][inside])
        assert hit.any(), (z, y, xx)
    # the blocked helper poisons the same voxels, every channel, in every storage type
    for dt in ("f32", "bf16", "f16"):
        k = R.kc(dt)
        t = R.poison_blocked(R.pack_blocked(x[:, :1].expand(2, 2 * k, d, h, w), dt), region)
        assert torch.equal(torch.isnan(R.unpack_blocked(t)), (~box).expand(2, 2 * k, d, h, w))
        assert bool((R.bits(t)[:, :, ~box] == -1).all())
