"""
compute_dtype="bf16x3" without a GPU: the plan accepts EXASPIM_DT_BF16X3, the packed image has
the documented size and holds every folded weight as a bf16 hi fragment and a bf16 lo fragment in
MFMA fragment order, and the Python surface knows the mode.
"""

import ctypes

import numpy as np
import pytest
import torch

import bf16x3_ref as X
import layer_ref as R
from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic

WIDTHS = [(32, 64, 128, 256, 512), (16, 32, 64, 128, 256), (4, 8, 16, 32, 64)]


def _pad(c):
    return (c + 31) // 32 * 32


def _convs(c, convt):
    """(ca_real, cb_real, cout_real) of the 17 MFMA convolutions (plan.cpp)."""
    h4 = c[4] if convt else c[4] // 2
    t = (lambda a, b: a) if convt else (lambda a, b: b)
    return [(c[0], 0, c[0]), (c[0], 0, c[1]), (c[1], 0, c[1]), (c[1], 0, c[2]), (c[2], 0, c[2]),
            (c[2], 0, c[3]), (c[3], 0, c[3]), (c[3], 0, h4), (h4, 0, h4),
            (c[3], t(c[4] // 2, h4), t(c[3], c[4] // 2)), (t(c[3], c[4] // 2), 0, t(c[3], c[3] // 2)),
            (c[2], c[3] // 2, t(c[2], c[3] // 2)), (t(c[2], c[3] // 2), 0, t(c[2], c[2] // 2)),
            (c[1], c[2] // 2, t(c[1], c[2] // 2)), (t(c[1], c[2] // 2), 0, t(c[1], c[1] // 2)),
            (c[0], c[1] // 2, t(c[0], c[1] // 2)), (t(c[0], c[1] // 2), 0, c[0])]


def _documented_bytes(c, oc, convt):
    """Two 16-bit fragments per padded weight; float32 bias, head, first layer and (UP_CONVT)
    transposed convolutions; every block aligned to 256 bytes."""
    al = lambda v: (v + 255) // 256 * 256   # noqa: E731
    c0p = _pad(c[0])
    n = al(27 * c0p * 4) + al(c0p * 4)
    for i, (ca, cb, co) in enumerate(_convs(c, convt)):
        if convt and i >= 9 and (i - 9) % 2 == 0:
            cin = c[4 - (i - 9) // 2]
            n += al(8 * _pad(cin) * _pad(cin // 2) * 4) + al(_pad(cin // 2) * 4)
        cin = _pad(ca) + (_pad(cb) if cb else 0)
        n += al(27 * cin * _pad(co) * 2 * 2) + al(_pad(co) * 4)
    return n + al(oc * c0p * 4) + al(oc * 4)


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("convt", [False, True])
def test_packed_bytes_is_the_documented_size(c, convt):
    lib = _native.lib()
    code = _native.DT_BF16X3 | (_native.UP_CONVT if convt else 0)
    got = lib.exaspim_unet_packed_bytes(_native.channels_array(c), 3, code)
    assert got != 0, _native.last_error()
    assert got == _documented_bytes(c, 3, convt)
    # the parameter vector does not depend on the compute dtype
    assert (lib.exaspim_unet_param_count(_native.channels_array(c), 3, code) ==
            lib.exaspim_unet_param_count(_native.channels_array(c), 3, code & ~0xff))


def test_unknown_dtype_codes_are_still_rejected():
    lib = _native.lib()
    ch = _native.channels_array(WIDTHS[0])
    assert lib.exaspim_unet_packed_bytes(ch, 3, 4) == 0
    assert "dtype" in _native.last_error()


@pytest.mark.parametrize("wm,trilinear", [(1, True), (0.125, True), (0.5, False)])
def test_pack_weights_round_trip(wm, trilinear):
    c = [max(1, int(round(v * wm))) for v in WIDTHS[0]]
    sd = synthetic.synth_state_dict(3, wm, seed=5, trilinear=trilinear)
    params = np.concatenate([v.reshape(-1).astype(np.float32) for k, v in sd.items()
                             if not k.endswith("num_batches_tracked")])
    lib = _native.lib()
    ch = _native.channels_array(c)
    images = {}
    for name, code in (("x3", _native.DT_BF16X3), ("f32", _native.DT_F32)):
        code |= 0 if trilinear else _native.UP_CONVT
        nbytes = lib.exaspim_unet_packed_bytes(ch, 3, code)
        img = np.zeros(nbytes, np.uint8)
        _native.check(lib.exaspim_unet_pack_weights(ch, 3, code, params.ctypes.data, params.size,
                                                    img.ctypes.data, nbytes), "pack")
        images[name] = img
    # same block sizes, and everything that is not a 3x3x3 MFMA convolution's weights is the float32
    # image's bytes: inc.0, biases, the head, ConvTranspose3d fragments
    assert images["x3"].size == images["f32"].size
    same = np.ones(images["x3"].size, bool)
    al = lambda v: (v + 255) // 256 * 256   # noqa: E731
    off = al(27 * _pad(c[0]) * 4) + al(_pad(c[0]) * 4)
    names = ["inc.double_conv.3"] + [f"down{l}.maxpool_conv.1.double_conv.{k}" for l in (1, 2, 3, 4) for k in (0, 3)] + \
            [f"up{l}.conv.double_conv.{k}" for l in (1, 2, 3, 4) for k in (0, 3)]
    for i, ((ca, cb, co), name) in enumerate(zip(_convs(c, not trilinear), names)):
        if not trilinear and i >= 9 and (i - 9) % 2 == 0:
            cin = c[4 - (i - 9) // 2]
            off += al(8 * _pad(cin) * _pad(cin // 2) * 4) + al(_pad(cin // 2) * 4)
        cap, cbp, cop = _pad(ca), (_pad(cb) if cb else 0), _pad(co)
        nbytes = 27 * (cap + cbp) * cop * 4
        same[off: off + nbytes] = False
        w_hi, w_lo = X.decode_weights(images["x3"], off, cap + cbp, cop)
        w64, _ = R.fold_bn64(sd, name)
        want = np.zeros((cop, cap + cbp, 27))
        want[:co, :ca] = w64[:, :ca]
        want[:co, cap: cap + cb] = w64[:, ca:]
        w32 = torch.from_numpy(want.astype(np.float32))
        hi, lo = X.split(w32)
        # hi is bf16(float32(folded weight)) bit for bit, lo the documented remainder
        assert np.array_equal(w_hi, hi.numpy()), name
        assert np.array_equal(w_lo, lo.numpy()), name
        # hi + lo reproduces the float32 weight to within one ulp of the lo part (2^-16 relative)
        err = np.abs(w_hi + w_lo - w32.numpy().astype(np.float64))
        assert (err <= np.abs(w32.numpy()) * 2.0 ** -16).all(), name
        off += al(nbytes) + al(cop * 4)
    assert np.array_equal(images["x3"][same], images["f32"][same])


def test_python_surface_knows_the_mode():
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    assert _native.DT_BF16X3 == 3 and _native.DTYPE_CODES["bf16x3"] == 3
    model = UNet3D(output_channels=3, compute_dtype="bf16x3")
    assert model.compute_dtype == "bf16x3" and model.active_dtype() == "bf16x3"
    assert not model.needs_resolution()
    with pytest.raises(ValueError):
        UNet3D(compute_dtype="bf16x2")
    # "auto" still decides between fp16 and float32 only
    assert UNet3D(compute_dtype="auto").active_dtype() == "fp32"


def test_header_documents_the_code():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "exaspim_affinity.h")).read()
    assert re.search(r"#define\s+EXASPIM_DT_BF16X3\s+3\b", text)
    assert re.search(r"#define\s+EXASPIM_ABI_VERSION\s+5\b", text)


def test_emulation_of_one_convolution_matches_the_float64_reference():
    """The CPU emulation behind the end-to-end tolerance (bf16x3_ref.conv3_x3) forms the same three
    products as the float64 reference of the per-layer tests."""
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((1, 32, 6, 6, 6), generator=gen)
    w = torch.randn((32, 32, 3, 3, 3), generator=gen) / 30
    b = torch.randn(32, generator=gen)
    w_hi, w_lo = X.split(w.reshape(32, 32, 27))
    acc, s = X.conv_ref(x, w_hi, w_lo, b)
    got = X.conv3_x3(x, w, b).to(torch.float64)
    assert ((got - acc).abs() <= X.conv_bound(s, 32) * 16).all()   # (torch's float32 sums: one step per product)
