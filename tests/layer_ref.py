"""
Float64 references and the checker for the per-layer tests (test_gpu_layers.py,
test_gpu_row_layers.py).

Plain helpers, no fixtures. Activations live in the library's blocked channels-last
layout, (N, C / KC, D, H, W, KC): one 32-byte record per voxel and channel chunk, KC = 16
channels in the 16-bit types and 8 in float32. Weights of an MFMA convolution are read
back out of a packed image of exaspim_unet_pack_weights in fragment order, so the
reference multiplies exactly the operands the kernel reads.
"""

import ctypes
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from aind_exaspim_neuron_segmentation_amd import _native

torch.set_num_threads(min(16, torch.get_num_threads()))

DTYPES = {"f32": _native.DT_F32, "bf16": _native.DT_BF16, "f16": _native.DT_F16}
STORAGE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SLOPE = 0.01

PROBE_PATH = os.path.join(os.path.dirname(_native.LIB_PATH), "libexaspim_layer_probe.so")


def es(dt):
    """Bytes per element of a storage type."""
    return 4 if dt == "f32" else 2


def kc(dt):
    """Channels per 32-byte chunk."""
    return 32 // es(dt)


# ---- storage rounding --------------------------------------------------------
def quantize(x, dt):
    """float64 -> storage type -> float64: RNE; f16 saturates at +-65504; NaN stays NaN."""
    x = torch.as_tensor(x, dtype=torch.float64)
    if dt == "f16":
        x = torch.where(torch.isnan(x), x, x.clamp(-65504.0, 65504.0))
    # through float32 first, as the kernels round their float32 values
    return x.to(torch.float32).to(STORAGE[dt]).to(torch.float64)


def leaky(x, slope=SLOPE):
    return torch.where(x >= 0, x, x * slope)


# ---- blocked layout ----------------------------------------------------------
def pack_blocked(x, dt):
    """(N, C, D, H, W) values -> blocked storage tensor (N, C/KC, D, H, W, KC) of the storage
    type (values are rounded to it; C must be a multiple of KC)."""
    x = torch.as_tensor(x)
    n, c, d, h, w = x.shape
    k = kc(dt)
    assert c % k == 0, (c, k)
    if dt == "f16":
        x = x.to(torch.float64).clamp(-65504.0, 65504.0)
    y = x.to(torch.float32).to(STORAGE[dt]).reshape(n, c // k, k, d, h, w)
    return y.permute(0, 1, 3, 4, 5, 2).contiguous()


def unpack_blocked(t):
    """Blocked storage tensor -> (N, C, D, H, W) float64."""
    n, cc, d, h, w, k = t.shape
    return t.permute(0, 1, 5, 2, 3, 4).reshape(n, cc * k, d, h, w).to(torch.float64)


def bits(t):
    """Raw integer view of a storage tensor (for bit-for-bit comparisons)."""
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


# ---- read footprint of a region launch -----------------------------------------
def grown_box(dhw, region):
    """bool (D, H, W): the region (org + ext, six numbers) grown by one voxel on every face and
    clipped to the patch -- the only source voxels the outputs in [org, org + ext) may depend on."""
    m = torch.zeros(tuple(int(v) for v in dhw), dtype=torch.bool)
    m[tuple(slice(max(0, o - 1), min(int(s), o + e + 1)) for o, e, s in zip(region[:3], region[3:], dhw))] = True
    return m


def poison_outside(x, region):
    """Copy of the (N, C, D, H, W) values with every channel outside grown_box set to NaN."""
    y = torch.as_tensor(x).clone()
    y[:, :, ~grown_box(y.shape[2:], region)] = float("nan")
    return y


def poison_blocked(t, region):
    """Sets, in place, every channel of a blocked source (N, C/KC, D, H, W, KC) outside grown_box to
    all-ones bits: a NaN in float32, IEEE half and bfloat16."""
    bits(t)[:, :, ~grown_box(t.shape[2:5], region)] = -1
    return t


# ---- packed weights ----------------------------------------------------------
def decode_storage(raw, dt):
    """uint8 bytes of the storage type -> float64 numpy array."""
    if dt == "f32":
        return raw.view(np.float32).astype(np.float64)
    if dt == "bf16":
        return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return raw.view(np.float16).astype(np.float64)


def decode_conv_weights(packed, w_off, cin, cout, dt):
    """A layer's weights in fragment order [chunk][tap 27][32-cout tile][lane 64][G] -> float64
    (cout, cin, 27), indexed by PADDED output and input channel (source A's channels, then B's).
    Lane l of a fragment holds cout 32 * tile + l % 32 and the G channels KC * chunk + G * (l // 32) + j."""
    g = 16 // es(dt)
    nchunks, ntiles = cin // (2 * g), cout // 32
    n = nchunks * 27 * ntiles * 64 * g
    vals = decode_storage(np.asarray(packed)[w_off: w_off + n * es(dt)], dt)
    frag = vals.reshape(nchunks, 27, ntiles, 2, 32, g)   # [c][t][tile][half][co][j]
    w = frag.transpose(2, 4, 0, 3, 5, 1).reshape(cout, cin, 27)   # [tile co][c half j][t]
    return w


def plan_conv(probe, channels, out_channels, dt, layer):
    """(ca_real, cb_real, ca, cb, cout_real, cout, w_off, b_off) of MFMA conv `layer`."""
    out = (ctypes.c_int64 * 8)()
    rc = probe.probe_plan_conv(_native.channels_array(channels), out_channels, DTYPES[dt], layer, out)
    assert rc == 0, probe.probe_last_error()
    return tuple(int(v) for v in out)


def fold_bn64(sd, prefix, eps=1e-5):
    """Conv3d + BatchNorm3d of a state dict folded in float64: W (cout, cin, 27), bias."""
    w = sd[prefix + ".weight"].astype(np.float64)
    cout, cin = w.shape[:2]
    bn = prefix.rsplit(".", 1)[0] + "." + str(int(prefix.rsplit(".", 1)[1]) + 1)
    g = sd[bn + ".weight"].astype(np.float64)
    beta = sd[bn + ".bias"].astype(np.float64)
    mu = sd[bn + ".running_mean"].astype(np.float64)
    var = sd[bn + ".running_var"].astype(np.float64)
    s = g / np.sqrt(var + eps)
    b = (sd[prefix + ".bias"].astype(np.float64) - mu) * s + beta
    return w.reshape(cout, cin, 27) * s[:, None, None], b


def round_like_plan(v, dt):
    """float64 -> float32 -> storage type (RNE; f16 saturating), as plan.cpp packs weights."""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    if dt == "f32":
        return v32.astype(np.float64)
    if dt == "f16":
        return np.clip(v32, -65504, 65504).astype(np.float16).astype(np.float64)
    return torch.from_numpy(v32).to(torch.bfloat16).to(torch.float64).numpy()


# ---- reference convolution and checker --------------------------------------
def conv_ref(x, w, b):
    """float64 3x3x3 convolution, padding 1: x (N, Cin, D, H, W), w (cout, cin, 27), b (cout).
    Returns the pre-activation acc and S = sum |w||x| + |b| per output voxel."""
    x = torch.as_tensor(x, dtype=torch.float64)
    w5 = torch.as_tensor(w, dtype=torch.float64).reshape(w.shape[0], w.shape[1], 3, 3, 3)
    b = torch.as_tensor(b, dtype=torch.float64)
    acc = F.conv3d(x, w5, b, padding=1)
    s = F.conv3d(x.abs(), w5.abs(), b.abs(), padding=1)
    return acc, s


def conv_bound(s, cin, dt, ksplit=1, taps=27):
    """Accumulation bound of the MFMA convolutions: (ceil(K / k) + ksplit + 4) 2^-24 S, K = taps * cin."""
    k = 2 if dt == "f32" else 16
    return (math.ceil(taps * cin / k) + ksplit + 4) * 2.0 ** -24 * s


def check_conv(got, acc, s, cin, dt, cout_real=None, ksplit=1, mask=None, exact_frac=0.99, nan_ok=None,
               taps=27, act=True, extra=None):
    """Asserts that every stored output equals Q(leaky(v)) for some |v - acc| <= bound, that (16-bit
    types) at least `exact_frac` of them equal Q(leaky(acc)) exactly and that padded output channels
    are exactly 0. got / acc / s: (N, C, D, H, W) float64; mask: bool voxels to check (default all);
    nan_ok: bool (N, C, D, H, W) where acc is NaN and the output must be NaN. taps: products per input
    channel (27; 8 phases of a transposed convolution); act: LeakyReLU or none; extra: an error term
    added to the bound (operand splitting), same shape as s."""
    f = leaky if act else (lambda v: v)
    got = torch.as_tensor(got, dtype=torch.float64)
    if mask is None:
        mask = torch.ones_like(got, dtype=torch.bool)
    cr = got.shape[1] if cout_real is None else cout_real
    pad = got[:, cr:][mask[:, cr:]]
    assert torch.all(pad == 0), f"padded output channels not 0: {pad[pad != 0][:8].tolist()}"
    g, a, sb = got[:, :cr], acc[:, :cr], s[:, :cr]
    m = mask[:, :cr]
    nan = torch.isnan(a)
    if nan_ok is not None:
        nan = nan | nan_ok[:, :cr]
    gn = torch.isnan(g)
    bad_nan = (gn != nan) & m
    assert not bad_nan.any(), (
        f"{int(bad_nan.sum())} outputs NaN where the reference is not (or the reverse), "
        f"first at {bad_nan.nonzero()[0].tolist()}")
    m = m & ~nan
    bound = conv_bound(sb, cin, dt, ksplit, taps)
    if extra is not None:
        bound = bound + extra[:, :cr]
    lo = quantize(f(a - bound), dt)
    hi = quantize(f(a + bound), dt)
    out = ((g < lo) | (g > hi)) & m
    if out.any():
        i = tuple(out.nonzero()[0].tolist())
        raise AssertionError(
            f"{int(out.sum())} of {int(m.sum())} outputs outside the accumulation bound; first at {list(i)}: "
            f"got {g[i].item()!r}, reference {a[i].item()!r} -> [{lo[i].item()!r}, {hi[i].item()!r}]")
    if dt != "f32" and int(m.sum()) > 0:
        exact = (g == quantize(f(a), dt)) & m
        frac = float(exact.sum()) / float(m.sum())
        assert frac >= exact_frac, f"only {frac:.4f} of the outputs are the correctly rounded reference"


def maxpool_ref(x):
    """2x2x2 max of float64 values, NaN propagating (torch max_pool3d)."""
    return F.max_pool3d(torch.as_tensor(x, dtype=torch.float64), 2)


# ---- operands of a row of overlapping patches ------------------------------------------
def _uniform_pm(shape, gen, lo=0.5):
    mag = lo + (1 - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)
    return mag * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).to(torch.float64)


def row_inputs(n, c, d, h, w, stride, gen):
    """(n, c, d, h, w) float64 inputs of n patches that are one row along x, `stride` voxels apart,
    as inc.3 sees them in row mode (ConvArgs::row_stride): cut from one strip, so neighbours agree on
    the columns they share, except each patch's own outermost x towards a neighbour (local x = 0 of
    patches 1 .. n-1, x = w-1 of patches 0 .. n-2), where inc.0's zero padding makes them differ.
    Those get fresh draws of twice the magnitude: an output computed in the wrong patch's frame is
    then far outside any accumulation bound."""
    strip = _uniform_pm((c, d, h, n * stride + (w - stride)), gen)
    x = torch.stack([strip[..., i * stride: i * stride + w].clone() for i in range(n)])
    x[1:, ..., 0] = 2 * _uniform_pm((n - 1, c, d, h), gen)
    x[:-1, ..., w - 1] = 2 * _uniform_pm((n - 1, c, d, h), gen)
    return x


def load_probe():
    lib = ctypes.CDLL(PROBE_PATH)
    vp, i32, f32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    sigs = {
        "probe_last_error": (ctypes.c_char_p, []),
        "probe_last_config": (ctypes.c_char_p, []),
        "probe_last_ksplit": (i32, []),
        "probe_last_layer_kernel": (ctypes.c_char_p, []),
        "probe_convt2": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        "probe_reset_config": (None, []),
        "probe_conv3x3x3": (i32, [i32, i32, vp, vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, f32,
                                  vp, vp, vp, sz, vp, vp, vp, i32, i32, vp]),
        "probe_conv_first": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp]),
        "probe_last_row": (i32, []),
        "probe_conv3x3x3_row": (i32, [i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, i32, vp]),
        "probe_conv_row_mode_ok": (i32, [i32, i32, i32, i32, i32, i32]),
        "probe_maxpool2_xcols": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "probe_maxpool2": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, vp]),
        "probe_upsample2": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "probe_upsample2_hi": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, i32, ctypes.c_int32 * 3, i32, i32, vp]),
        "probe_head": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "probe_plan_conv": (i32, [ctypes.c_int32 * 5, i32, i32, i32, ctypes.POINTER(ctypes.c_int64)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib
