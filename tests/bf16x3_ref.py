"""
Helpers of the compute_dtype="bf16x3" tests (no fixtures, no tests).

The mode (include/exaspim_affinity.h, EXASPIM_DT_BF16X3) splits both operands of every 3x3x3
MFMA convolution, hi = bf16(v) rounded to nearest even and lo = bf16(v - float(hi)), and sums
the three products w_hi x_hi, w_hi x_lo, w_lo x_hi in float32. Here: the split, the packed
fragment order of the split weights, the float64 reference of the same three products with
its derived accumulation bound, and a CPU emulation of the whole network in that arithmetic
(the reference path of oracle/reference_path.py with each such convolution replaced).
"""

import math

import numpy as np
import torch
import torch.nn.functional as F

DT_BF16X3 = 3
SLOPE = 0.01


def split(v):
    """float32-valued tensor (any float dtype) -> (hi, lo), float64 tensors holding bf16 values."""
    v32 = torch.as_tensor(v).to(torch.float32)
    hi = v32.to(torch.bfloat16)
    lo = (v32 - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.to(torch.float64), lo.to(torch.float64)


def _bf16_bits(t):
    return t.to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def encode_parts(w_hi, w_lo):
    """(cout, cin, 27) bf16-valued hi and lo parts, padded channels -> uint16 numpy image in the packed
    order [16-channel chunk][tap 27][32-cout tile][hi, lo][lane 64][8]: lane l holds cout 32 tile + l % 32
    and channels 16 chunk + 8 (l // 32) + j."""
    cout, cin, taps = w_hi.shape
    parts = []
    for part in (torch.as_tensor(w_hi), torch.as_tensor(w_lo)):
        frag = part.reshape(cout // 32, 32, cin // 16, 2, 8, taps).permute(2, 5, 0, 3, 1, 4)   # [c][t][tile][half][co][j]
        parts.append(torch.from_numpy(_bf16_bits(frag)).reshape(frag.shape))
    return torch.stack(parts, dim=3).contiguous().numpy().reshape(-1)    # [c][t][tile][part][half][co][j]


def encode_weights(w):
    """The same from float32-valued weights, split by the rule above."""
    return encode_parts(*split(torch.as_tensor(w)))


def decode_weights(packed, w_off, cin, cout):
    """Packed image (uint8 numpy) -> (w_hi, w_lo), float64 numpy (cout, cin, 27) by padded channel."""
    n = 27 * cin * cout * 2
    raw = np.asarray(packed)[w_off: w_off + 2 * n].view(np.uint16)
    vals = (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    frag = vals.reshape(cin // 16, 27, cout // 32, 2, 2, 32, 8)   # [c][t][tile][part][half][co][j]
    w = frag.transpose(3, 2, 5, 0, 4, 6, 1).reshape(2, cout, cin, 27)
    return w[0], w[1]


def leaky(x, slope=SLOPE):
    return torch.where(x >= 0, x, x * slope)


def conv_ref(x, w_hi, w_lo, b):
    """float64 reference of the three products: conv(x_hi + x_lo, w_hi) + conv(x_hi, w_lo) + b, and
    S = the same sum over absolute values. x (N, Cin, D, H, W) float32-valued, w_* (cout, cin, 27)."""
    x_hi, x_lo = split(x)
    w5 = lambda w: torch.as_tensor(w, dtype=torch.float64).reshape(w.shape[0], w.shape[1], 3, 3, 3)   # noqa: E731
    b = torch.as_tensor(b, dtype=torch.float64)
    acc = F.conv3d(x_hi + x_lo, w5(w_hi), b, padding=1) + F.conv3d(x_hi, w5(w_lo), None, padding=1)
    s = (F.conv3d(x_hi.abs() + x_lo.abs(), w5(w_hi).abs(), b.abs(), padding=1) +
         F.conv3d(x_hi.abs(), w5(w_lo).abs(), None, padding=1))
    return acc, s


def conv_bound(s, cin, ksplit=1):
    """layer_ref.conv_bound with three MFMAs per K = 16 step: (3 ceil(27 cin / 16) + ksplit + 4) 2^-24 S."""
    return (3 * math.ceil(27 * cin / 16) + ksplit + 4) * 2.0 ** -24 * s


def check_conv(got, acc, s, cin, cout_real=None, ksplit=1, mask=None):
    """Every float32 output equals f32(leaky(v)) for some |v - acc| <= bound; padded output channels
    are exactly 0; an output is NaN exactly where the reference is."""
    f32 = lambda v: v.to(torch.float32).to(torch.float64)   # noqa: E731
    got = torch.as_tensor(got, dtype=torch.float64)
    if mask is None:
        mask = torch.ones_like(got, dtype=torch.bool)
    cr = got.shape[1] if cout_real is None else cout_real
    pad = got[:, cr:][mask[:, cr:]]
    assert torch.all(pad == 0), f"padded output channels not 0: {pad[pad != 0][:8].tolist()}"
    g, a, sb, m = got[:, :cr], acc[:, :cr], s[:, :cr], mask[:, :cr]
    nan = torch.isnan(a)
    bad_nan = (torch.isnan(g) != nan) & m
    assert not bad_nan.any(), f"{int(bad_nan.sum())} outputs NaN where the reference is not (or the reverse)"
    m = m & ~nan
    bound = conv_bound(sb, cin, ksplit)
    lo, hi = f32(leaky(a - bound)), f32(leaky(a + bound))
    out = ((g < lo) | (g > hi)) & m
    rel = float(((g - leaky(a)).abs() / bound.clamp_min(1e-300))[m].max()) if bool(m.any()) else 0.0
    print(f"bf16x3 conv: max |got - ref| / bound = {rel:.3f} over {int(m.sum())} outputs")
    if out.any():
        i = tuple(out.nonzero()[0].tolist())
        raise AssertionError(
            f"{int(out.sum())} of {int(m.sum())} outputs outside the accumulation bound; first at {list(i)}: "
            f"got {g[i].item()!r}, reference {a[i].item()!r} -> [{lo[i].item()!r}, {hi[i].item()!r}]")


# ---- CPU emulation of the network in bf16x3 arithmetic ------------------------------------------
def conv3_x3(x, w, b):
    """3x3x3 convolution, padding 1, in the mode's arithmetic: float32 operands split by the rule
    above, the three products summed in float32 (the order of the sum is torch's, not the kernel's)."""
    x = x.to(torch.float32)
    w = w.to(torch.float32)
    x_hi = x.to(torch.bfloat16).to(torch.float32)
    x_lo = (x - x_hi).to(torch.bfloat16).to(torch.float32)
    w_hi = w.to(torch.bfloat16).to(torch.float32)
    w_lo = (w - w_hi).to(torch.bfloat16).to(torch.float32)
    y = F.conv3d(x_hi, w_hi, None, padding=1)
    y = y + F.conv3d(x_lo, w_hi, None, padding=1)
    y = y + F.conv3d(x_hi, w_lo, None, padding=1)
    return y + b.to(torch.float32).reshape(1, -1, 1, 1, 1)


def _fold(sd, conv, bn, eps=1e-5):
    """Conv3d + eval BatchNorm3d folded in float64, rounded to float32 (as the library packs them)."""
    t = lambda k: torch.as_tensor(np.asarray(sd[k]), dtype=torch.float64)   # noqa: E731
    s = t(bn + ".weight") / torch.sqrt(t(bn + ".running_var") + eps)
    w = t(conv + ".weight") * s.reshape(-1, 1, 1, 1, 1)
    b = (t(conv + ".bias") - t(bn + ".running_mean")) * s + t(bn + ".bias")
    return w.to(torch.float32), b.to(torch.float32)


def emulate_unet(sd, x, trilinear=True):
    """UNet3D.forward (logits) on float32 x (N, 1, D, H, W) with every 3x3x3 convolution after inc.0
    in bf16x3 arithmetic; everything else float32, like the engine."""
    x = torch.as_tensor(x, dtype=torch.float32)

    def double_conv(x, prefix, first_plain=False):
        w, b = _fold(sd, prefix + ".0", prefix + ".1")
        x = F.conv3d(x, w, b, padding=1) if first_plain else conv3_x3(x, w, b)
        x = F.leaky_relu(x, SLOPE)
        w, b = _fold(sd, prefix + ".3", prefix + ".4")
        return F.leaky_relu(conv3_x3(x, w, b), SLOPE)

    t32 = lambda k: torch.as_tensor(np.asarray(sd[k]), dtype=torch.float32)   # noqa: E731
    with torch.no_grad():
        skips = [double_conv(x, "inc.double_conv", first_plain=True)]
        for l in range(1, 5):
            skips.append(double_conv(F.max_pool3d(skips[-1], 2), f"down{l}.maxpool_conv.1.double_conv"))
        y = skips[4]
        for l in range(1, 5):
            if trilinear:
                y = F.interpolate(y, scale_factor=2, mode="trilinear", align_corners=True)
            else:
                y = F.conv_transpose3d(y, t32(f"up{l}.up.weight"), t32(f"up{l}.up.bias"), stride=2)
            y = double_conv(torch.cat([skips[4 - l], y], dim=1), f"up{l}.conv.double_conv")
        return F.conv3d(y, t32("outc.conv.weight"), t32("outc.conv.bias"))
