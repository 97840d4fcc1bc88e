"""
Per-layer tests of the bf16x3 convolution (conv3d.hip: conv3x3x3_x3, launch_typed_x3,
launch_thin_typed_x3) through the layer probe, against a float64 reference OF THE SAME THREE
PRODUCTS: conv64(x_hi + x_lo, w_hi) + conv64(x_hi, w_lo) + bias, then LeakyReLU, with the
operands split by the documented rule (bf16x3_ref.py). What remains is float32 accumulation
order, so the bound is derived, not measured: layer_ref.conv_bound with three MFMAs per K = 16
step, (3 ceil(27 cin / 16) + ksplit + 4) 2^-24 S. Every configuration the dispatch can take is
asserted through last_conv_launch() and the last test checks that all are reached.
"""

import ctypes
import math
import re

import numpy as np
import pytest
import torch

import bf16x3_ref as X
import layer_ref as R
from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic

pytestmark = pytest.mark.gpu

DT = X.DT_BF16X3
SENTINEL = 0x5A
E_INVALID = -1


@pytest.fixture(scope="module")
def probe():
    import __graft_entry__

    __graft_entry__.build()
    assert torch.cuda.is_available()
    return R.load_probe()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _uniform_pm(shape, gen, lo=0.5):
    mag = lo + (1 - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)
    return mag * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).to(torch.float64)


def _f32(v):
    return torch.as_tensor(v, dtype=torch.float64).to(torch.float32).to(torch.float64)


def _config(probe):
    cfg = probe.probe_last_config().decode()
    m = re.match(r".*\b(launch_\w+)\(.*\[(.*)\]$", cfg)
    assert m, cfg
    params = dict(p.strip().split(" = ") for p in m.group(2).split(","))
    return m.group(1), tuple(int(params[k]) for k in ("TZ", "TY", "TX", "WAVES_M", "WAVES_N", "MT", "NT", "MINW", "PD"))


class Layer:
    """Random float32 operands of one convolution; padded channels carry zero weights and bias."""

    def __init__(self, ca, cb, cout, n, d, h, w, seed=0, ca_real=None, cb_real=None, cout_real=None,
                 x=None, w_hi=None, w_lo=None, bias=None):
        gen = torch.Generator().manual_seed(seed)
        self.ca, self.cb, self.cout, self.shape = ca, cb, cout, (n, d, h, w)
        ca_real = ca if ca_real is None else ca_real
        cb_real = cb if cb_real is None else cb_real
        self.cout_real = cout if cout_real is None else cout_real
        if x is None:
            x = _uniform_pm((n, ca + cb, d, h, w), gen)
            x[:, ca_real:ca] = 0
            x[:, ca + cb_real:] = 0
        self.x = _f32(x)
        if w_hi is None:
            weights = _uniform_pm((cout, ca + cb, 27), gen) / math.sqrt(27 * (ca_real + cb_real))
            weights[self.cout_real:] = 0
            weights[:, ca_real:ca] = 0
            weights[:, ca + cb_real:] = 0
            w_hi, w_lo = X.split(_f32(weights))
        self.w_hi, self.w_lo = torch.as_tensor(w_hi), torch.as_tensor(w_lo)
        if bias is None:
            bias = torch.zeros(cout, dtype=torch.float64)
            bias[: self.cout_real] = 0.5 * _uniform_pm((self.cout_real,), gen, lo=0.0)
        self.b = _f32(bias)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = X.conv_ref(self.x, self.w_hi, self.w_lo, self.b)
        return self._ref

    def packed_weights(self):
        img = X.encode_parts(self.w_hi, self.w_lo)
        hi, lo = X.decode_weights(img.view(np.uint8), 0, self.ca + self.cb, self.cout)
        assert np.array_equal(hi, self.w_hi.numpy()) and np.array_equal(lo, self.w_lo.numpy())
        return torch.from_numpy(img.view(np.int16).copy())

    def packed_sources(self, src_poison=None):
        xa = R.pack_blocked(self.x[:, : self.ca], "f32")
        xb = R.pack_blocked(self.x[:, self.ca:], "f32") if self.cb else None
        if src_poison is not None:
            R.poison_blocked(xa, src_poison)
            if xb is not None:
                R.poison_blocked(xb, src_poison)
        return xa.to("cuda"), xb.to("cuda") if xb is not None else None

    def run(self, probe, region=None, partial=False, thin=False, dst=None, expect_rc=0, pool=False, head=False,
            ca_arg=None, src_poison=None):
        """src_poison: a region (org + ext); every channel of both packed sources outside that box grown
        by one voxel is set to NaN bits (layer_ref.poison_blocked)."""
        n, d, h, w = self.shape
        dev = "cuda"
        xa, xb = self.packed_sources(src_poison)
        wt = self.packed_weights().to(dev)
        bt = self.b.to(torch.float32).to(dev)
        if dst is None:
            dst = torch.zeros((n, self.cout // 8, d, h, w, 8), dtype=torch.float32, device=dev)
            if region is not None:
                dst.view(torch.uint8).fill_(SENTINEL)
        part, part_bytes = None, 0
        if partial:
            part_bytes = 4 * d * h * w * self.cout * 4
            part = torch.empty(n * part_bytes // 4, dtype=torch.float32, device=dev)
        pdst = torch.zeros((n, self.cout // 8, d // 2, h // 2, w // 2, 8), dtype=torch.float32, device=dev) if pool else None
        hw = hb = hout = None
        if head:
            hw, hb = torch.ones(32, device=dev), torch.zeros(1, device=dev)
            hout = torch.zeros((n, 1, d, h, w), device=dev)
        reg = (ctypes.c_int32 * 6)(*(region if region is not None else (0,) * 6))
        probe.probe_reset_config()
        torch.cuda.synchronize()
        rc = probe.probe_conv3x3x3(int(thin), DT, _ptr(xa), _ptr(xb), self.ca if ca_arg is None else ca_arg, self.cb, _ptr(wt), _ptr(bt),
                                   _ptr(dst), self.cout, n, d, h, w, X.SLOPE, reg, _ptr(pdst), _ptr(part),
                                   part_bytes, _ptr(hw), _ptr(hb), _ptr(hout), int(head), 0, None)
        if expect_rc:
            assert rc == expect_rc, rc
            return probe.probe_last_error().decode()
        assert rc == 0, probe.probe_last_error().decode()
        torch.cuda.synchronize()
        self.launcher, self.config = _config(probe)
        self.ksplit = probe.probe_last_ksplit()
        self.dst_dev = dst
        self.dst = dst.cpu()
        return self

    def check(self, mask=None):
        acc, s = self.ref()
        X.check_conv(R.unpack_blocked(self.dst), acc, s, self.ca + self.cb, cout_real=self.cout_real,
                     ksplit=self.ksplit, mask=mask)


# configurations of launch_typed_x3 / launch_thin_typed_x3: (TZ, TY, TX, WAVES_M, WAVES_N, MT, NT, MINW, PD)
A = (4, 8, 16, 4, 1, 4, 1, 2, 3)
B = (2, 8, 16, 4, 1, 2, 2, 2, 3)
C2 = (4, 4, 24, 4, 1, 3, 2, 2, 1)
C1 = (4, 4, 24, 4, 1, 3, 1, 2, 3)
E = (4, 4, 12, 2, 1, 3, 1, 2, 3)
F22 = (4, 4, 12, 2, 2, 3, 2, 2, 2)
F21 = (4, 4, 12, 2, 2, 3, 1, 2, 3)
H = (6, 6, 6, 4, 1, 2, 1, 2, 3)
TY2 = (8, 2, 16, 4, 1, 2, 1, 2, 3)
TX2 = (8, 16, 2, 4, 1, 2, 1, 2, 3)
ALL_CONFIGS = {A, B, C2, C1, E, F22, F21, H, TY2, TX2}

# (ca, cb, cout, d, h, w, expected configuration): every branch, every pyramid level's tile, cout 32 / 64 /
# 128 / 256, one and two sources, odd multiples of 16 (48, 80) and sizes that are none (40, 10, 5, 3)
BRANCHES = [
    (32, 0, 32, 6, 8, 96, A),
    (32, 32, 32, 6, 4, 48, A),
    (64, 0, 32, 5, 8, 32, A),
    (32, 0, 32, 7, 8, 16, A),
    (32, 0, 32, 4, 16, 80, A),
    (32, 0, 64, 6, 8, 96, B),
    (32, 32, 64, 5, 8, 48, B),
    (64, 0, 128, 4, 8, 32, B),
    (32, 0, 256, 3, 8, 16, B),
    (32, 0, 32, 4, 4, 24, C1),
    (64, 0, 64, 6, 4, 24, C2),
    (32, 0, 32, 5, 5, 40, C1),
    (32, 32, 128, 4, 4, 40, C2),
    (32, 0, 32, 4, 4, 12, E),
    (64, 0, 64, 4, 4, 12, F21),
    (32, 32, 128, 4, 4, 12, F22),
    (64, 0, 256, 4, 4, 10, E),
    (32, 0, 96, 5, 4, 10, E),
    (64, 0, 32, 6, 6, 6, H),
    (32, 32, 256, 6, 6, 6, H),
    (32, 0, 64, 3, 5, 4, H),
]


@pytest.mark.parametrize("case", BRANCHES, ids=lambda c: "x".join(map(str, c[:6])))
def test_dispatch_branch(probe, case):
    ca, cb, cout, d, h, w, config = case
    L = Layer(ca, cb, cout, 2, d, h, w, seed=sum(case[:6])).run(probe)
    assert (L.launcher, L.config) == ("launch_x3", config)
    assert L.ksplit == 1
    L.check()


# ---- the 17 MFMA convolutions of the network, weights from the product's packed image ------
LEVEL_SHAPE = {0: (4, 8, 96), 1: (4, 8, 48), 2: (4, 4, 24), 3: (4, 4, 12), 4: (6, 6, 6)}
LAYER_LEVEL = [0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0]   # inc.3, down1.0 .. up4.3


def packed_image(wm, seed, code=DT):
    widths = [max(1, int(round(c * wm))) for c in (32, 64, 128, 256, 512)]
    sd = synthetic.synth_state_dict(3, wm, seed=seed)
    params = np.concatenate([v.reshape(-1).astype(np.float32) for k, v in sd.items()
                             if not k.endswith("num_batches_tracked")])
    lib = _native.lib()
    ch = _native.channels_array(widths)
    nbytes = lib.exaspim_unet_packed_bytes(ch, 3, code)
    packed = np.zeros(nbytes, np.uint8)
    _native.check(lib.exaspim_unet_pack_weights(ch, 3, code, params.ctypes.data, params.size,
                                                packed.ctypes.data, nbytes), "pack")
    return widths, packed, sd


@pytest.mark.parametrize("wm", [1, 0.5])
def test_network_layers(probe, wm):
    widths, packed, _ = packed_image(wm, seed=17)
    for layer in range(17):
        out = (ctypes.c_int64 * 8)()
        assert probe.probe_plan_conv(_native.channels_array(widths), 3, DT, layer, out) == 0
        ca_r, cb_r, ca, cb, co_r, co, w_off, b_off = (int(v) for v in out)
        w_hi, w_lo = X.decode_weights(packed, w_off, ca + cb, co)
        b = torch.from_numpy(packed[b_off: b_off + 4 * co].view(np.float32).astype(np.float64))
        d, h, wd = LEVEL_SHAPE[LAYER_LEVEL[layer]]
        L = Layer(ca, cb, co, 1, d, h, wd, seed=layer, ca_real=ca_r, cb_real=cb_r, cout_real=co_r,
                  w_hi=torch.from_numpy(w_hi), w_lo=torch.from_numpy(w_lo), bias=b)
        L.run(probe)
        try:
            L.check()
        except AssertionError as e:
            raise AssertionError(f"layer {layer} ({ca_r}+{cb_r} -> {co_r}): {e}") from None


# ---- split-K ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 12, 12), (6, 6, 6)])
def test_split_k(probe, shape):
    L0 = Layer(64, 0, 64, 2, *shape, seed=9).run(probe)
    assert L0.ksplit == 1
    L0.check()
    L1 = Layer(64, 0, 64, 2, *shape, seed=9).run(probe, partial=True)
    assert L1.ksplit > 1, (L1.config, L1.ksplit)
    L1.check()
    # the split is a function of the layer and the patch size, not of the batch: a patch alone gets the same bits
    L2 = Layer(64, 0, 64, 1, *shape, x=L1.x[:1], w_hi=L1.w_hi, w_lo=L1.w_lo, bias=L1.b).run(probe, partial=True)
    assert L2.ksplit == L1.ksplit
    assert torch.equal(R.bits(L2.dst), R.bits(L1.dst[:1]))


# ---- regions and thin tiles ------------------------------------------------------------------
def _region_mask(shape, region):
    m = torch.zeros(shape, dtype=torch.bool)
    (oz, oy, ox), (ez, ey, ex) = region[:3], region[3:]
    m[:, :, oz: oz + ez, oy: oy + ey, ox: ox + ex] = True
    return m


def _blocked_mask(m):
    n, c, d, h, w = m.shape
    return m.reshape(n, c // 8, 8, d, h, w).permute(0, 1, 3, 4, 5, 2)


def _check_region(L, region):
    shape = (L.shape[0], L.cout) + L.shape[1:]
    m = _region_mask(shape, region)
    raw = L.dst.contiguous().view(torch.uint8).reshape(L.dst.shape + (4,))
    touched = (raw[~_blocked_mask(m)] != SENTINEL).any(-1)
    assert not touched.any(), f"{int(touched.sum())} values outside the region written"
    L.check(mask=m)


REGIONS = [
    # (thin, ca, cout, d, h, w, org + ext, expected configuration)
    (0, 32, 32, 8, 12, 48, (1, 2, 3, 6, 9, 40), A),
    (0, 32, 64, 6, 12, 32, (2, 0, 5, 3, 12, 20), B),
    (0, 32, 32, 6, 8, 24, (1, 1, 2, 4, 6, 19), C1),
    (0, 64, 64, 6, 10, 12, (0, 3, 1, 5, 5, 10), F21),
    (1, 32, 32, 12, 16, 32, (0, 6, 0, 12, 2, 16), TY2),
    (1, 64, 32, 12, 16, 32, (2, 13, 8, 8, 3, 20), TY2),
    (1, 32, 32, 12, 16, 32, (1, 0, 30, 8, 16, 2), TX2),
    (1, 32, 32, 12, 16, 32, (5, 0, 3, 4, 11, 4), TX2),
]


@pytest.mark.parametrize("case", REGIONS, ids=lambda c: f"thin{c[0]}-" + "-".join(map(str, c[6])))
def test_region(probe, case):
    thin, ca, cout, d, h, w, region, config = case
    L = Layer(ca, 0, cout, 2, d, h, w, seed=sum(region)).run(probe, region=region, thin=bool(thin))
    assert L.config == config
    _check_region(L, region)


def test_trimmed_region_with_thin_remainders_has_the_bits_of_the_whole_patch(probe):
    """A trimmed region as the engine cuts it: whole main tiles, then the y remainder (every x of
    the region) and the x remainder (rows of the main part) on thin tiles. Every kept voxel has
    the bits of the untrimmed launch; nothing else is written."""
    n, d, h, w = 2, 10, 24, 48
    org, ext = (3, 3, 3), (4, 18, 36)          # 18 = 2 x 8 + 2, 36 = 2 x 16 + 4
    whole = Layer(32, 32, 32, n, d, h, w, seed=11).run(probe)
    assert whole.config == A
    whole.check()
    L = Layer(32, 32, 32, n, d, h, w, seed=11)
    main = org + (ext[0], 16, 32)
    L.run(probe, region=main)
    assert L.config == A
    L.run(probe, region=(org[0], org[1] + 16, org[2], ext[0], 2, 36), thin=True, dst=L.dst_dev)
    assert L.config == TY2
    L.run(probe, region=(org[0], org[1], org[2] + 32, ext[0], 16, 4), thin=True, dst=L.dst_dev)
    assert L.config == TX2
    m = _blocked_mask(_region_mask((n, 32, d, h, w), org + ext))
    assert torch.equal(R.bits(L.dst)[m], R.bits(whole.dst)[m])
    raw = L.dst.contiguous().view(torch.uint8).reshape(L.dst.shape + (4,))
    assert (raw[~m] == SENTINEL).all()


def _trimmed_with_remainders(probe, poisoned):
    """The three launches of the engine's trimmed region (main tiles, y remainder, x remainder) into one
    sentinel-filled dst; poisoned: each launch's sources are NaN outside its own region's grown box."""
    n, d, h, w = 2, 10, 24, 48
    org, ext = (3, 3, 3), (4, 18, 36)
    L = Layer(32, 32, 32, n, d, h, w, seed=11)
    parts = [(org + (ext[0], 16, 32), False, A), ((org[0], org[1] + 16, org[2], ext[0], 2, 36), True, TY2),
             ((org[0], org[1], org[2] + 32, ext[0], 16, 4), True, TX2)]
    dst = None
    for region, thin, config in parts:
        L.run(probe, region=region, thin=thin, dst=dst, src_poison=region if poisoned else None)
        assert L.config == config
        dst = L.dst_dev
    return L, org + ext


@pytest.mark.parametrize("case", REGIONS + ["trimmed"],
                         ids=lambda c: c if isinstance(c, str) else f"thin{c[0]}-" + "-".join(map(str, c[6])))
def test_region_reads_only_its_grown_box(probe, case):
    """The engine's contract for a region launch: outputs in [org, org + ext) depend on source voxels of
    that box grown by one voxel only. Everything else of both sources is NaN here, and the region still
    passes the float64 check, has the bits of the launch on the clean sources, and holds no NaN -- for
    every region and thin-tile case above and the trimmed region cut into main tiles and remainders."""
    if case == "trimmed":
        clean, region = _trimmed_with_remainders(probe, poisoned=False)
        L, _ = _trimmed_with_remainders(probe, poisoned=True)
    else:
        thin, ca, cout, d, h, w, region, config = case
        clean = Layer(ca, 0, cout, 2, d, h, w, seed=sum(region)).run(probe, region=region, thin=bool(thin))
        L = Layer(ca, 0, cout, 2, d, h, w, seed=sum(region)).run(probe, region=region, thin=bool(thin),
                                                                 src_poison=region)
        assert L.config == config == clean.config
    _check_region(L, region)
    m = _region_mask((L.shape[0], L.cout) + L.shape[1:], region)
    assert not torch.isnan(R.unpack_blocked(L.dst)[m]).any(), "NaN inside the region"
    mb = _blocked_mask(m)
    differ = R.bits(L.dst)[mb] != R.bits(clean.dst)[mb]
    assert not differ.any(), f"{int(differ.sum())} of {int(mb.sum())} outputs of the region changed with the poison"


# ---- edge data -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(32, 0, 32, 6, 8, 32), (32, 32, 64, 4, 8, 32), (64, 0, 64, 4, 4, 24)],
                         ids=lambda c: "x".join(map(str, c)))
def test_activations_beyond_half_range(probe, case):
    """|x| in 1e5 .. 1e6, beyond anything fp16 holds: float32's range is kept and the error bound
    is the same relative one."""
    ca, cb, cout, d, h, w = case
    gen = torch.Generator().manual_seed(5)
    x = _uniform_pm((1, ca + cb, d, h, w), gen, lo=0.1) * 1e6
    L = Layer(ca, cb, cout, 1, d, h, w, seed=6, x=x).run(probe)
    L.check()
    got = R.unpack_blocked(L.dst)
    assert torch.isfinite(got).all() and float(got.abs().max()) > 65504


def test_tiny_operands(probe):
    gen = torch.Generator().manual_seed(3)
    x = _uniform_pm((1, 32, 4, 8, 32), gen) * 2.0 ** -40
    L = Layer(32, 0, 32, 1, 4, 8, 32, seed=8, x=x, bias=torch.zeros(32)).run(probe)
    L.check()
    assert float(R.unpack_blocked(L.dst).abs().max()) > 0


@pytest.mark.parametrize("case", [(32, 32, 6, 8, 32), (32, 64, 4, 8, 32), (32, 64, 4, 4, 24), (32, 64, 6, 6, 6)],
                         ids=lambda c: "x".join(map(str, c)))
def test_nan_input_voxel(probe, case):
    """A NaN activation propagates like in the float32 kernel: to every real output channel of
    the 27 voxels whose window holds it, and nowhere else."""
    ca, cout, d, h, w = case
    gen = torch.Generator().manual_seed(4)
    x = _uniform_pm((1, ca, d, h, w), gen)
    z, y, xx = d // 2, 1, w - 2
    x[0, 5, z, y, xx] = float("nan")
    L = Layer(ca, 0, cout, 1, d, h, w, x=x, cout_real=cout - 2).run(probe)
    got = R.unpack_blocked(L.dst)
    win = torch.zeros_like(got, dtype=torch.bool)
    win[:, :, max(0, z - 1): z + 2, max(0, y - 1): y + 2, max(0, xx - 1): xx + 2] = True
    assert torch.isnan(got[:, : cout - 2][win[:, : cout - 2]]).all(), "a NaN in the window came out finite"
    assert not torch.isnan(got[~win]).any(), "NaN outside the NaN voxel's window"
    L.check(mask=~win)


def test_repeated_launches_are_bit_identical(probe):
    a = Layer(32, 32, 64, 3, 6, 8, 48, seed=2).run(probe)
    b = Layer(32, 32, 64, 3, 6, 8, 48, seed=2).run(probe)
    assert torch.equal(R.bits(a.dst), R.bits(b.dst))


# ---- what the mode does not have -------------------------------------------------------------
def test_rejected_arguments(probe):
    assert "max-pool" in Layer(32, 0, 32, 1, 8, 8, 32).run(probe, pool=True, expect_rc=E_INVALID)
    assert "head" in Layer(32, 0, 32, 1, 8, 8, 32).run(probe, head=True, expect_rc=E_INVALID)
    # a single float32 chunk plane is no pair
    assert "not padded" in Layer(32, 0, 32, 1, 8, 8, 32).run(probe, ca_arg=8, expect_rc=E_INVALID)


def test_float32_layers_take_the_code(probe):
    """Max-pool through the probe with the bf16x3 code runs the float32 kernel (same bits)."""
    gen = torch.Generator().manual_seed(6)
    x = _f32(_uniform_pm((2, 16, 6, 8, 10), gen))
    src = R.pack_blocked(x, "f32").cuda()
    outs = []
    for code in (_native.DT_F32, DT):
        dst = torch.zeros((2, 2, 3, 4, 5, 8), dtype=torch.float32, device="cuda")
        assert probe.probe_maxpool2(code, _ptr(src), _ptr(dst), 2, 6, 8, 10, 16, None) == 0
        torch.cuda.synchronize()
        outs.append(dst.cpu())
    assert torch.equal(R.bits(outs[0]), R.bits(outs[1]))
    assert torch.equal(R.unpack_blocked(outs[1]), R.maxpool_ref(x))


# ---- coverage of the dispatch ----------------------------------------------------------------
def test_dispatch_coverage(probe):
    """Every configuration launch_typed_x3 / launch_thin_typed_x3 can produce is reached by the
    tables above, and no other."""
    hit = set()
    for ca, cb, cout, d, h, w, _ in BRANCHES:
        hit.add(Layer(ca, cb, cout, 1, d, h, w).run(probe).config)
    for thin, ca, cout, d, h, w, region, _ in REGIONS:
        hit.add(Layer(ca, 0, cout, 1, d, h, w).run(probe, region=region, thin=bool(thin)).config)
    assert hit == ALL_CONFIGS, (sorted(ALL_CONFIGS - hit), sorted(hit - ALL_CONFIGS))
