"""
Per-layer tests of the HIP layer kernels against float64 references (layer_ref.py).

Every dispatch path of the 3x3x3 convolution (conv3d.hip: launch_typed, launch_thin_typed,
launch_cfg) is driven on its own through the test-only probe library
(libexaspim_layer_probe.so) and checked voxel by voxel against a float64 convolution of the
very operands the kernel reads, in float32, bf16 and fp16. The probe reports which
configuration each launch took; the last test asserts that the cases cover every one the
dispatch can produce.
"""

import ctypes
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R
from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic

pytestmark = pytest.mark.gpu

DTS = ["f32", "bf16", "f16"]
E_INVALID = -1   # EXASPIM_E_INVALID
SENTINEL = 0x5A   # byte pattern of voxels a region launch must leave untouched

@pytest.fixture(scope="module")
def probe():
    import __graft_entry__

    __graft_entry__.build()
    assert torch.cuda.is_available()
    return R.load_probe()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _record(probe, dt):
    cfg = probe.probe_last_config().decode()
    m = re.match(r".*\b(launch_\w+)\(.*\[(.*)\]$", cfg)
    assert m, cfg
    params = tuple(p.strip() for p in m.group(2).split(",") if not p.strip().startswith("Tag ="))
    return m.group(1), dict(p.split(" = ") for p in params), (dt, m.group(1), params)


def _uniform_pm(shape, gen, lo=0.5):
    mag = lo + (1 - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)
    return mag * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).to(torch.float64)


def encode_conv_weights(w, dt):
    """float64 (cout, cin, 27), padded channels -> fragment-order storage tensor (inverse of
    layer_ref.decode_conv_weights)."""
    cout, cin, taps = w.shape   # taps: 27, or the 8 phases of a transposed convolution
    g = 16 // R.es(dt)
    frag = np.asarray(w).reshape(cout // 32, 32, cin // (2 * g), 2, g, taps).transpose(2, 5, 0, 3, 1, 4)
    t = torch.from_numpy(np.ascontiguousarray(frag).reshape(-1))
    if dt == "f16":
        t = t.clamp(-65504, 65504)
    return t.to(torch.float32).to(R.STORAGE[dt])


class Layer:
    """Random operands of one convolution (padded channels carry zero weights and bias)."""

    def __init__(self, dt, ca, cb, cout, n, d, h, w, seed=0, ca_real=None, cb_real=None, cout_real=None,
                 x=None, weights=None, bias=None):
        gen = torch.Generator().manual_seed(seed)
        self.dt, self.ca, self.cb, self.cout = dt, ca, cb, cout
        self.shape = (n, d, h, w)
        ca_real = ca if ca_real is None else ca_real
        cb_real = cb if cb_real is None else cb_real
        self.cout_real = cout if cout_real is None else cout_real
        if x is None:
            x = _uniform_pm((n, ca + cb, d, h, w), gen)
            x[:, ca_real:ca] = 0
            x[:, ca + cb_real:] = 0
        self.x = R.quantize(x, dt)
        if weights is None:
            # scaled so that activations stay O(1) whatever the fan-in
            weights = _uniform_pm((cout, ca + cb, 27), gen) / math.sqrt(27 * (ca_real + cb_real))
            weights[self.cout_real:] = 0
            weights[:, ca_real:ca] = 0
            weights[:, ca + cb_real:] = 0
        self.w = R.quantize(weights, dt)
        if bias is None:
            bias = torch.zeros(cout, dtype=torch.float64)
            bias[: self.cout_real] = 0.5 * _uniform_pm((self.cout_real,), gen, lo=0.0)
        self.b = torch.as_tensor(bias, dtype=torch.float64).to(torch.float32).to(torch.float64)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = R.conv_ref(self.x, self.w, self.b)
        return self._ref

    def run(self, probe, region=None, pool=False, partial=False, head=None, thin=False, dst_fill=None,
            expect_rc=0, ca_arg=None, src_poison=None):
        """src_poison: a region (org + ext); every channel of both packed sources outside that box grown
        by one voxel is set to NaN bits (layer_ref.poison_blocked)."""
        dt, (n, d, h, w) = self.dt, self.shape
        k = R.kc(dt)
        dev = "cuda"
        xa = R.pack_blocked(self.x[:, : self.ca], dt)
        xb = R.pack_blocked(self.x[:, self.ca:], dt) if self.cb else None
        if src_poison is not None:
            R.poison_blocked(xa, src_poison)
            if xb is not None:
                R.poison_blocked(xb, src_poison)
        xa = xa.to(dev)
        xb = xb.to(dev) if xb is not None else None
        wt = encode_conv_weights(self.w.numpy(), dt).to(dev)
        bt = self.b.to(torch.float32).to(dev)
        dst = torch.zeros((n, self.cout // k, d, h, w, k), dtype=R.STORAGE[dt], device=dev)
        if dst_fill is not None:
            R.bits(dst).view(torch.uint8).fill_(dst_fill)
        pdst = None
        if pool:
            pdst = torch.full((n, self.cout // k, d // 2, h // 2, w // 2, k), 7.0, dtype=R.STORAGE[dt], device=dev)
        part, part_bytes = None, 0
        if partial:
            part_bytes = 4 * d * h * w * self.cout * 4
            part = torch.empty(n * part_bytes // 4, dtype=torch.float32, device=dev)
        hw = hb = hout = None
        oc = sig = 0
        if head is not None:
            oc, sig, hw64, hb64 = head
            hw = hw64.to(torch.float32).to(dev)
            hb = hb64.to(torch.float32).to(dev)
            hout = torch.full((n, oc, d, h, w), float("nan"), dtype=torch.float32, device=dev)
        reg = (ctypes.c_int32 * 6)(*(region if region is not None else (0,) * 6))
        probe.probe_reset_config()
        torch.cuda.synchronize()
        rc = probe.probe_conv3x3x3(int(thin), R.DTYPES[dt], _ptr(xa), _ptr(xb), self.ca if ca_arg is None else ca_arg, self.cb, _ptr(wt), _ptr(bt),
                                   _ptr(dst), self.cout, n, d, h, w, R.SLOPE, reg, _ptr(pdst), _ptr(part),
                                   part_bytes, _ptr(hw), _ptr(hb), _ptr(hout), oc, sig, None)
        if expect_rc:
            assert rc == expect_rc, rc
            return probe.probe_last_error().decode()
        assert rc == 0, probe.probe_last_error().decode()
        torch.cuda.synchronize()
        self.launcher, self.params, self.config = _record(probe, dt)
        self.ksplit = probe.probe_last_ksplit()
        self.dst = dst.cpu()
        self.pool = pdst.cpu() if pool else None
        self.head = hout.cpu().to(torch.float64) if head is not None else None
        return self

    def check(self, mask=None, nan_ok=None):
        acc, s = self.ref()
        R.check_conv(R.unpack_blocked(self.dst), acc, s, self.ca + self.cb, self.dt, cout_real=self.cout_real,
                     ksplit=self.ksplit, mask=mask, nan_ok=nan_ok)


# ---- every launch_typed branch ------------------------------------------------
# (ca, cb, cout, d, h, w, expected launcher, expected tile (TZ, TY, TX))
BRANCHES = [
    (32, 0, 32, 6, 8, 96, "launch_zpipe", (6, 8, 16)),
    (32, 0, 32, 4, 8, 96, "launch_zpipe", (4, 8, 16)),
    (32, 32, 32, 6, 4, 48, "launch_zpipe", (6, 8, 16)),
    (64, 0, 32, 5, 8, 32, "launch_zpipe", (4, 8, 16)),
    (32, 0, 32, 12, 8, 16, "launch_zpipe", (6, 8, 16)),
    (32, 0, 32, 7, 8, 16, "launch_zpipe", (4, 8, 16)),
    (32, 0, 64, 6, 8, 96, "launch_cfg", (4, 8, 16)),
    (32, 32, 64, 5, 8, 48, "launch_cfg", (4, 8, 16)),
    (64, 0, 128, 4, 8, 32, "launch_cfg", (4, 8, 16)),
    (32, 0, 64, 6, 8, 16, "launch_cfg", (4, 8, 16)),
    (32, 0, 32, 4, 4, 24, "launch_cfg", (4, 4, 24)),
    (64, 0, 64, 6, 4, 24, "launch_cfg", (4, 4, 24)),
    (32, 0, 32, 5, 5, 40, "launch_cfg", (4, 4, 24)),
    (32, 0, 128, 4, 4, 40, "launch_cfg", (4, 4, 24)),
    (32, 0, 32, 4, 4, 12, "launch_cfg", (4, 4, 12)),
    (64, 0, 64, 4, 4, 12, "launch_cfg", (4, 4, 12)),
    (32, 32, 128, 4, 4, 12, "launch_cfg", (4, 4, 12)),
    (64, 0, 256, 4, 4, 10, "launch_cfg", (4, 4, 12)),
    (32, 0, 96, 5, 4, 10, "launch_cfg", (4, 4, 12)),
    (64, 0, 32, 6, 6, 6, "launch_cfg", (6, 6, 6)),
    (32, 0, 256, 6, 6, 6, "launch_cfg", (6, 6, 6)),
    (32, 0, 64, 3, 5, 4, "launch_cfg", (6, 6, 6)),
]


def _tile(params):
    return tuple(int(params[k]) for k in ("TZ", "TY", "TX"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", BRANCHES, ids=lambda c: "x".join(map(str, c[:6])))
def test_dispatch_branch(probe, dt, case):
    ca, cb, cout, d, h, w, launcher, tile = case
    L = Layer(dt, ca, cb, cout, 1, d, h, w, seed=sum(case[:6])).run(probe)
    assert (L.launcher, _tile(L.params)) == (launcher, tile), (L.launcher, L.params)
    assert L.ksplit == 1
    L.check()


# ---- the 17 MFMA convolutions of the network, weights from the product's packed image ------
LEVEL_SHAPE = {0: (4, 4, 96), 1: (4, 4, 48), 2: (4, 4, 24), 3: (4, 4, 12), 4: (6, 6, 6)}
LAYER_LEVEL = [0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0]   # inc.3, down1.0 .. up4.3


def _packed_image(dt, wm, seed):
    widths = [max(1, int(round(c * wm))) for c in (32, 64, 128, 256, 512)]
    sd = synthetic.synth_state_dict(3, wm, seed=seed)
    params = np.concatenate([v.reshape(-1).astype(np.float32) for k, v in sd.items()
                             if not k.endswith("num_batches_tracked")])
    lib = _native.lib()
    ch = _native.channels_array(widths)
    nbytes = lib.exaspim_unet_packed_bytes(ch, 3, R.DTYPES[dt])
    packed = np.zeros(nbytes, np.uint8)
    _native.check(lib.exaspim_unet_pack_weights(ch, 3, R.DTYPES[dt], params.ctypes.data, params.size,
                                                packed.ctypes.data, nbytes), "pack")
    return widths, packed


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("wm", [1, 0.5, 0.125])
def test_network_layers(probe, dt, wm):
    widths, packed = _packed_image(dt, wm, seed=17)
    for layer in range(17):
        ca_r, cb_r, ca, cb, co_r, co, w_off, b_off = R.plan_conv(probe, widths, 3, dt, layer)
        w = torch.from_numpy(R.decode_conv_weights(packed, w_off, ca + cb, co, dt))
        b = torch.from_numpy(packed[b_off: b_off + 4 * co].view(np.float32).astype(np.float64))
        d, h, wd = LEVEL_SHAPE[LAYER_LEVEL[layer]]
        L = Layer(dt, ca, cb, co, 1, d, h, wd, seed=layer, ca_real=ca_r, cb_real=cb_r, cout_real=co_r,
                  weights=w, bias=b)
        L.run(probe)
        try:
            L.check()
        except AssertionError as e:
            raise AssertionError(f"layer {layer} ({ca_r}+{cb_r} -> {co_r}): {e}") from None


# ---- fused max-pool -----------------------------------------------------------
POOLED = [
    (32, 0, 32, 6, 8, 96, ("f32", "bf16", "f16")),
    (32, 32, 32, 4, 8, 32, ("f32", "bf16", "f16")),
    (32, 0, 64, 4, 8, 32, ("bf16", "f16")),
    (32, 0, 32, 4, 4, 24, ("bf16", "f16")),
    (32, 0, 64, 4, 4, 24, ("bf16", "f16")),
    (32, 0, 32, 4, 4, 12, ("bf16", "f16")),
    (32, 0, 64, 4, 4, 12, ("bf16", "f16")),
    (32, 0, 128, 4, 4, 12, ("bf16", "f16")),
    (32, 0, 256, 4, 4, 12, ("bf16", "f16")),
]


def _check_pool_of_dst(L):
    got = R.unpack_blocked(L.pool)
    want = R.maxpool_ref(R.unpack_blocked(L.dst))
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(got[ok], want[ok]), (got[ok] != want[ok]).nonzero()[:4]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", POOLED, ids=lambda c: "x".join(map(str, c[:6])))
def test_fused_pool(probe, dt, case):
    ca, cb, cout, d, h, w, dts = case
    if dt not in dts:
        L = Layer(dt, ca, cb, cout, 1, d, h, w)
        assert "max-pool" in L.run(probe, pool=True, expect_rc=E_INVALID)
        return
    L = Layer(dt, ca, cb, cout, 2, d, h, w, seed=3).run(probe, pool=True)
    assert L.params.get("POOL") == "true", L.params
    L.check()
    _check_pool_of_dst(L)


# ---- fused head -----------------------------------------------------------------
HEAD_DEPTHS = [(12, 6), (8, 4), (10, 5)]   # (d, planes per tile): 6-, 4- and 5-plane head tiles


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("oc", [1, 2, 3, 4])
@pytest.mark.parametrize("d,tz", HEAD_DEPTHS)
def test_fused_head(probe, dt, oc, d, tz):
    gen = torch.Generator().manual_seed(oc * 100 + d)
    hw = _uniform_pm((oc, 32), gen) / 4
    hb = _uniform_pm((oc,), gen, lo=0.0)
    for sig in (0, 1):
        L = Layer(dt, 32, 32, 32, 1, d, 8, 32, seed=oc, cout_real=30)
        L.run(probe, head=(oc, sig, hw, hb))
        assert (L.launcher, int(L.params["TZ"]), int(L.params["HEAD"])) == ("launch_zpipe", tz, oc)
        acc, s = L.ref()
        act = R.leaky(acc)
        bound = R.conv_bound(s, 64, dt)   # |leaky(v) - leaky(acc)| <= |v - acc|
        hw32 = hw.to(torch.float32).to(torch.float64)
        hb32 = hb.to(torch.float32).to(torch.float64)
        pre = torch.einsum("oc,ncdhw->nodhw", hw32, act) + hb32[None, :, None, None, None]
        tol = (torch.einsum("oc,ncdhw->nodhw", hw32.abs(), bound) +
               (32 + 4) * 2.0 ** -24 * (torch.einsum("oc,ncdhw->nodhw", hw32.abs(), act.abs()) +
                                        hb32.abs()[None, :, None, None, None]))
        want = torch.sigmoid(pre) if sig else pre
        if sig:   # sigmoid is 1/4-Lipschitz; expf and the division add a few float32 roundings
            tol = tol / 4 + 2.0 ** -21 * want.abs() + 2.0 ** -40
        err = (L.head - want).abs()
        assert torch.all(err <= tol), f"sig={sig}: max err {float(err.max()):.3e} (tol {float(tol.max()):.3e})"


# ---- split-K -----------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(12, 12, 12), (6, 6, 6)])
def test_split_k(probe, dt, shape):
    ca = 64 if dt != "f32" else 32
    L0 = Layer(dt, ca, 0, 64, 2, *shape, seed=9).run(probe)
    assert L0.ksplit == 1
    L0.check()
    L1 = Layer(dt, ca, 0, 64, 2, *shape, seed=9).run(probe, partial=True)
    assert L1.ksplit > 1, (L1.params, L1.ksplit)
    L1.check()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_split_k_with_pool(probe, dt):
    L = Layer(dt, 64, 0, 64, 2, 12, 12, 12, seed=4).run(probe, pool=True, partial=True)
    assert L.ksplit > 1 and L.params["POOL"] == "true", (L.params, L.ksplit)
    L.check()
    _check_pool_of_dst(L)


# ---- regions and thin tiles ----------------------------------------------------------
def _region_mask(shape, region):
    n, c, d, h, w = shape
    m = torch.zeros(shape, dtype=torch.bool)
    (oz, oy, ox), (ez, ey, ex) = region[:3], region[3:]
    m[:, :, oz: oz + ez, oy: oy + ey, ox: ox + ex] = True
    return m


def _check_region(L, region):
    shape = (L.shape[0], L.cout) + L.shape[1:]
    m = _region_mask(shape, region)
    raw = R.bits(L.dst).view(torch.uint8).reshape(L.dst.shape + (-1,))
    outside = ~m.reshape(shape[0], L.cout // R.kc(L.dt), R.kc(L.dt), *shape[2:]).permute(0, 1, 3, 4, 5, 2)
    touched = (raw[outside] != SENTINEL).any(-1)
    assert not touched.any(), f"{int(touched.sum())} values outside the region written"
    L.check(mask=m)


REGIONS = [
    # (thin, ca, cout, d, h, w, org + ext, expected launcher tile)
    (0, 32, 32, 8, 12, 48, (1, 2, 3, 6, 9, 40), (4, 8, 16)),
    (0, 32, 64, 6, 12, 32, (2, 0, 5, 3, 12, 20), (4, 8, 16)),
    (0, 32, 32, 6, 8, 24, (1, 1, 2, 4, 6, 19), (4, 4, 24)),
    (0, 64, 64, 6, 10, 12, (0, 3, 1, 5, 5, 10), (4, 4, 12)),
    (1, 32, 32, 12, 16, 32, (0, 6, 0, 12, 2, 16), (12, 2, 16)),
    (1, 32, 32, 12, 16, 32, (2, 13, 8, 8, 2, 16), (8, 2, 16)),
    (1, 32, 32, 12, 16, 32, (3, 0, 16, 4, 2, 16), (4, 2, 16)),
    (1, 32, 32, 12, 16, 32, (1, 0, 30, 8, 16, 2), (8, 16, 2)),
    (1, 32, 32, 12, 16, 32, (5, 0, 0, 4, 16, 2), (4, 16, 2)),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", REGIONS, ids=lambda c: f"thin{c[0]}-" + "-".join(map(str, c[6])))
def test_region(probe, dt, case):
    thin, ca, cout, d, h, w, region, tile = case
    L = Layer(dt, ca, 0, cout, 2, d, h, w, seed=sum(region)).run(probe, region=region, thin=bool(thin),
                                                                 dst_fill=SENTINEL)
    assert _tile(L.params) == tile, L.params
    _check_region(L, region)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", REGIONS, ids=lambda c: f"thin{c[0]}-" + "-".join(map(str, c[6])))
def test_region_reads_only_its_grown_box(probe, dt, case):
    """The engine's contract for a region launch: outputs in [org, org + ext) depend on source voxels of
    that box grown by one voxel only. Everything else of the source is NaN here, and the region still
    passes the float64 check, has the bits of the launch on the clean source, and holds no NaN."""
    thin, ca, cout, d, h, w, region, tile = case
    kw = dict(region=region, thin=bool(thin), dst_fill=SENTINEL)
    clean = Layer(dt, ca, 0, cout, 2, d, h, w, seed=sum(region)).run(probe, **kw)
    L = Layer(dt, ca, 0, cout, 2, d, h, w, seed=sum(region)).run(probe, src_poison=region, **kw)
    assert _tile(L.params) == tile and L.config == clean.config, L.params
    _check_region(L, region)
    m = _region_mask((2, cout, d, h, w), region)
    k = R.kc(dt)
    mb = m.reshape(2, cout // k, k, d, h, w).permute(0, 1, 3, 4, 5, 2)
    assert not torch.isnan(R.unpack_blocked(L.dst)[m]).any(), "NaN inside the region"
    differ = R.bits(L.dst)[mb] != R.bits(clean.dst)[mb]
    assert not differ.any(), f"{int(differ.sum())} of {int(mb.sum())} outputs of the region changed with the poison"


# ---- persistent tile walk ---------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_persistent_tile_walk(probe, dt, delta):
    # launch_zpipe: 32-cout slices, MINW = 2 -> max(8, 2 * CUs / slices // 8 * 8) workgroups;
    # a 4 x 8 x 16 patch is one tile
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wgs = max(8, 2 * cus // 8 * 8)
    n = wgs + delta
    L = Layer(dt, 32, 0, 32, n, 4, 8, 16, seed=delta + 5).run(probe)
    assert int(L.params["TZ"]) == 4
    keep = [0, n - 2, n - 1]
    acc, s = R.conv_ref(L.x[keep], L.w, L.b)
    R.check_conv(R.unpack_blocked(L.dst[keep]), acc, s, 32, dt)


# ---- edge data ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_sparse_input(probe, dt):
    gen = torch.Generator().manual_seed(1)
    x = _uniform_pm((1, 32, 6, 8, 32), gen)
    x[torch.rand(x.shape, generator=gen) < 0.97] = 0
    L = Layer(dt, 32, 0, 32, 1, 6, 8, 32, x=x).run(probe)
    L.check()


@pytest.mark.parametrize("dt", DTS)
def test_saturating_accumulators(probe, dt):
    gen = torch.Generator().manual_seed(2)
    x = 45000 * (0.5 + 0.5 * torch.rand((1, 32, 4, 8, 32), generator=gen, dtype=torch.float64))
    w = _uniform_pm((32, 32, 27), gen)
    w[0] = w[0].abs()
    w[1] = -w[1].abs()
    L = Layer(dt, 32, 0, 32, 1, 4, 8, 32, x=x, weights=w).run(probe)
    L.check()
    got = R.unpack_blocked(L.dst)
    if dt == "f16":   # interior voxels: all 27 taps, |acc| > 65504 / slope
        inner = got[:, :, 1:-1, 1:-1, 1:-1]
        assert (inner[:, 0] == 65504).all() and (inner[:, 1] == -65504).all()
    assert not torch.isinf(got).any()


@pytest.mark.parametrize("dt", DTS)
def test_subnormal_outputs(probe, dt):
    # products of 2^-10-scale operands (normal in every type) sum to float32 accumulators whose
    # activations lie in the fp16 subnormal range (< 2^-14). The float32 -> fp16 conversion keeps
    # denormals (the fp16 / fp64 denormal mode of the shader MODE register is on by default), so
    # the reference models no flushing.
    gen = torch.Generator().manual_seed(3)
    x = _uniform_pm((1, 32, 4, 8, 32), gen) * 2.0 ** -9
    w = _uniform_pm((32, 32, 27), gen) * 2.0 ** -9
    L = Layer(dt, 32, 0, 32, 1, 4, 8, 32, x=x, weights=w, bias=torch.zeros(32)).run(probe)
    L.check()
    if dt == "f16":
        got = R.unpack_blocked(L.dst)
        sub = (got != 0) & (got.abs() < 2.0 ** -14)
        assert sub.float().mean() > 0.2


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", [(32, 32, 6, 8, 32), (32, 64, 4, 4, 24), (32, 64, 6, 6, 6)],
                         ids=lambda c: "x".join(map(str, c)))
def test_nan_input_voxel(probe, dt, case):
    ca, cout, d, h, w = case
    gen = torch.Generator().manual_seed(4)
    x = _uniform_pm((1, ca, d, h, w), gen)
    z, y, xx = d // 2, 1, w - 2
    x[0, 5, z, y, xx] = float("nan")
    # with the fused pool where the dispatch has one: the NaN must reach the pooled voxel too
    pool = w > 6 and (dt != "f32" or cout % 64 != 0)
    L = Layer(dt, ca, 0, cout, 1, d, h, w, x=x, cout_real=cout - 2).run(probe, pool=pool)
    if pool:
        _check_pool_of_dst(L)
        assert torch.isnan(R.unpack_blocked(L.pool)[0, 0, z // 2, y // 2, xx // 2])
    got = R.unpack_blocked(L.dst)
    win = torch.zeros_like(got, dtype=torch.bool)
    win[:, :, max(0, z - 1): z + 2, max(0, y - 1): y + 2, max(0, xx - 1): xx + 2] = True
    real = got[:, : cout - 2]
    assert torch.isnan(real[win[:, : cout - 2]]).all(), "a NaN in the window came out finite"
    assert not torch.isnan(got[~win]).any(), "NaN outside the NaN voxel's window"
    # every other output passes the checker; padded channels are 0 outside the window
    L.check(mask=~win)


# ---- non-MFMA kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_maxpool2_nan_exact(probe, dt):
    gen = torch.Generator().manual_seed(6)
    k = R.kc(dt)
    x = R.quantize(_uniform_pm((2, 2 * k, 6, 8, 10), gen), dt)
    x[0, 1, 0, 0, 0] = float("nan")
    x[1, 3, 3, 5, 7] = -float("nan")
    x[1, k, 5, 7, 9] = float("nan")
    src = R.pack_blocked(x, dt).cuda()
    if dt != "f32":   # a negative NaN's sign bit as well
        R.bits(src)[1, 0, 3, 5, 7, 3] |= -0x8000
    dst = torch.zeros((2, 2, 3, 4, 5, k), dtype=R.STORAGE[dt], device="cuda")
    assert probe.probe_maxpool2(R.DTYPES[dt], _ptr(src), _ptr(dst), 2, 6, 8, 10, 2 * k, None) == 0
    torch.cuda.synchronize()
    got = R.unpack_blocked(dst.cpu())
    want = R.maxpool_ref(x)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), torch.isnan(got).sum()
    ok = ~torch.isnan(want)
    assert torch.equal(got[ok], want[ok])


def _lerp_matrix(n):
    """(2n, n) float64 weights of align_corners=True linear x2 interpolation along one axis, from
    ATen's float32 coordinates: scale = (n - 1) / (2n - 1), src = scale * o (rounded), i0 = floor,
    lambda = src - i0 (rounded), weights (1 - lambda, lambda) (rounded)."""
    f = np.float32
    scale = f(n - 1) / f(2 * n - 1) if n > 1 else f(0)
    m = np.zeros((2 * n, n))
    for o in range(2 * n):
        s = f(scale * f(o))
        i0 = min(int(np.floor(s)), n - 1)
        i1 = min(i0 + 1, n - 1)
        l1 = min(max(f(s - f(i0)), f(0)), f(1))
        m[o, i0] += float(f(f(1) - l1))
        m[o, i1] += float(l1)
    return torch.from_numpy(m)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["plain", "per_thread", "auto"])
@pytest.mark.parametrize("d,margin", [(6, 0), (16, 4), (18, 4), (7, 0)])
def test_upsample2(probe, dt, mode, d, margin):
    gen = torch.Generator().manual_seed(d)
    k = R.kc(dt)
    h, w = 6, 8
    x = R.quantize(_uniform_pm((1, 2 * k, d, h, w), gen), dt)
    src = R.pack_blocked(x, dt).cuda()
    dst = torch.zeros((1, 2, 2 * d, 2 * h, 2 * w, k), dtype=R.STORAGE[dt], device="cuda")
    rc = probe.probe_upsample2(R.DTYPES[dt], _ptr(src), _ptr(dst), 1, d, h, w, 2 * k, margin,
                               int(mode == "plain"), int(mode == "per_thread"), None)
    assert rc == 0, probe.probe_last_error()
    torch.cuda.synchronize()
    kernel = probe.probe_last_layer_kernel().decode()
    if mode == "plain":
        assert kernel == "upsample2"
    elif margin >= 4:   # nzp = d - margin pairs of output planes: runs of 12 (d 16) or 14 (d 18)
        assert kernel == ("upsample2_pipe" if mode == "per_thread" else f"upsample2_strip{d - margin}"), kernel
    else:
        assert kernel in ("upsample2_pipe", "upsample2"), kernel
    got = R.unpack_blocked(dst.cpu())
    m = margin
    sl = (slice(None), slice(None), slice(m, 2 * d - m), slice(m, 2 * h - m), slice(m, 2 * w - m))
    # Not bit for bit with ATen's trilinear kernel on the device: measured on MI355X, up to 2/3 of
    # the float32 outputs differ from it by 1 - 2 ulp (sums nested and contracted differently).
    # The reference takes ATen's
    # float32 coordinate arithmetic (_lerp_matrix) and sums in float64; the kernel must lie within
    # 8 float32 roundings of max |source| of it, then the storage cast.
    up64 = torch.einsum("ai,bj,ck,nqijk->nqabc", _lerp_matrix(d), _lerp_matrix(h),
                        _lerp_matrix(w), x)
    e = 8 * 2.0 ** -24 * x.abs().max()
    lo, hi = R.quantize(up64 - e, dt), R.quantize(up64 + e, dt)
    bad = (got[sl] < lo[sl]) | (got[sl] > hi[sl])
    assert not bad.any(), (f"{int(bad.sum())} of {bad.numel()} outside the bound, max |diff| "
                           f"{float((got[sl] - up64[sl]).abs().max()):.3e}")
    if dt != "f32":   # and the storage cast is the correctly rounded one for nearly all
        exact = got[sl] == R.quantize(up64, dt)[sl]
        assert exact.double().mean() >= 0.99


# The level-0 upsampling of the trimmed and clipped forward at shapes with more than one workgroup, two images and
# the high-face margins engine.hip derives from keep_hi. Per case: (d, h, w) of the source, margin, margin_hi, the
# kernel the launcher must pick when left to itself, and -- where that is the strip kernel -- per axis the first
# output index it leaves alone (hy and hx as given; along z the widest margin <= margin_hi[0] with whole runs).
UPS_HI_CASES = {
    # 12 pairs of 24 x 24 columns x 2 groups = 576 items: three workgroups along y, the later ones with image0 > 0
    "16x16x16 m4": ((16, 16, 16), 4, None, "upsample2_strip12", (28, 28, 28)),
    "32x16x16 m4": ((32, 16, 16), 4, None, "upsample2_strip14", (60, 28, 28)),       # 28 pairs: two runs of 14
    "24x16x16 m6": ((24, 16, 16), 6, None, "upsample2_pipe", None),                  # 18 pairs: no whole run
    # z margin 20 leaves 22 planes, 11 pairs; 19 leaves 23 planes in 12 pairs, one run, the last pair of one plane
    "24x16x16 m6 hi 20,14,10": ((24, 16, 16), 6, (20, 14, 10), "upsample2_strip12", (29, 18, 22)),
    "24x16x16 m6 hi z": ((24, 16, 16), 6, (20, 0, 0), "upsample2_strip12", (29, 26, 26)),
    # no z margin in [6, 6] gives whole runs, as given or symmetric: the superset on the per-thread pipeline
    "24x16x16 m6 hi y": ((24, 16, 16), 6, (0, 14, 0), "upsample2_pipe", None),
    # odd extents: the last row pair has one row (ny = 17), nx = 19; along z margin 5 leaves 23 planes in 12 pairs
    "16x16x16 m4 hi y,x odd": ((16, 16, 16), 4, (0, 11, 9), "upsample2_strip12", (28, 21, 23)),
    "16x16x16 m4 hi odd": ((16, 16, 16), 4, (9, 11, 9), "upsample2_strip12", (27, 21, 23)),
    # a workgroup's 128 (row pair, column) items span two row pairs of 152 columns: four source rows of 80 x 2
    # pieces = 640 > the 512 of an LDS slot
    "16x8x80 m4": ((16, 8, 80), 4, None, "upsample2_pipe", None),
}


def _axis_mask(dims, lo, hi):
    """bool (D, H, W): lo[i] <= index < hi[i] on every axis."""
    m = torch.ones(dims, dtype=torch.bool)
    for axis, (n, a, b) in enumerate(zip(dims, lo, hi)):
        idx = torch.arange(n)
        shape = [1, 1, 1]
        shape[axis] = n
        m &= ((idx >= a) & (idx < b)).reshape(shape)
    return m


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(UPS_HI_CASES))
def test_upsample2_many_workgroups_and_high_margins(probe, dt, case):
    (d, h, w), margin, margin_hi, auto_kernel, skipped = UPS_HI_CASES[case]
    gen = torch.Generator().manual_seed(d * h * w + margin)
    k = R.kc(dt)
    n = 2
    x = R.quantize(_uniform_pm((n, 2 * k, d, h, w), gen), dt)      # two images of two channel chunks
    src = R.pack_blocked(x, dt).cuda()
    dims = (2 * d, 2 * h, 2 * w)
    word = {4: 0x5A5A5A5A, 2: 0x5A5A}[R.es(dt)]
    # test_upsample2's reference and bound
    up64 = torch.einsum("ai,bj,ck,nqijk->nqabc", _lerp_matrix(d), _lerp_matrix(h), _lerp_matrix(w), x)
    e = 8 * 2.0 ** -24 * x.abs().max()
    lo, hi = R.quantize(up64 - e, dt), R.quantize(up64 + e, dt)
    rounded = R.quantize(up64, dt)
    mhi = [margin] * 3 if margin_hi is None else [max(margin, v) for v in margin_hi]
    assert all(margin <= v < s - margin for v, s in zip(mhi, dims))
    required = _axis_mask(dims, [margin] * 3, [s - v for s, v in zip(dims, mhi)])
    box = _axis_mask(dims, [margin] * 3, [s - margin for s in dims])
    assert int(required.sum()) > 0 and bool((required & ~box).sum() == 0)
    results = {}
    for mode in ("plain", "per_thread", "auto"):
        dst = torch.empty((n, 2) + dims + (k,), dtype=R.STORAGE[dt], device="cuda")
        R.bits(dst).fill_(word)
        flags = (int(mode == "plain"), int(mode == "per_thread"))
        if margin_hi is None:
            rc = probe.probe_upsample2(R.DTYPES[dt], _ptr(src), _ptr(dst), n, d, h, w, 2 * k, margin, *flags, None)
        else:
            rc = probe.probe_upsample2_hi(R.DTYPES[dt], _ptr(src), _ptr(dst), n, d, h, w, 2 * k, margin,
                                          (ctypes.c_int32 * 3)(*margin_hi), *flags, None)
        assert rc == 0, (mode, probe.probe_last_error())
        torch.cuda.synchronize()
        kernel = probe.probe_last_layer_kernel().decode()
        assert kernel == {"plain": "upsample2", "per_thread": "upsample2_pipe", "auto": auto_kernel}[mode], (mode, kernel)
        host = dst.cpu()
        got = R.unpack_blocked(host)
        untouched = R.unpack_blocked(R.bits(host)) == word
        results[mode] = R.unpack_blocked(R.bits(host))[:, :, required]
        good = (got >= lo) & (got <= hi)
        bad = ~good[:, :, required]
        assert not bad.any(), (f"{mode}: {int(bad.sum())} of {bad.numel()} needed outputs outside the bound, max |diff| "
                               f"{float((got - up64)[:, :, required].abs().max()):.3e}")
        optional = box & ~required
        bad = ~(good | untouched)[:, :, optional]
        assert not bad.any(), f"{mode}: {int(bad.sum())} outputs beyond margin_hi neither left alone nor within the bound"
        assert bool(untouched[:, :, ~box].all()), f"{mode}: outputs within the margin were written"
        if mode == "auto" and skipped is not None:     # the strip kernel stops where it says it does
            written = _axis_mask(dims, [margin] * 3, skipped)
            assert bool(untouched[:, :, ~written].all()), "the strip kernel wrote beyond its high margins"
            assert not bool(untouched[:, :, written].any()), "the strip kernel left outputs inside its margins alone"
        if dt != "f32":   # the storage cast is the correctly rounded one for nearly all
            exact = (got == rounded)[:, :, required]
            assert exact.double().mean() >= 0.99, mode
    for mode in ("per_thread", "auto"):
        differ = results[mode] != results["plain"]
        assert not differ.any(), f"{mode} and plain differ in {int(differ.sum())} of {differ.numel()} needed outputs"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("oc", [1, 3, 4])
def test_head_kernel(probe, dt, oc):
    gen = torch.Generator().manual_seed(oc)
    c0p = 32
    x = R.quantize(_uniform_pm((2, c0p, 4, 6, 10), gen), dt)
    w = _uniform_pm((oc, c0p), gen).to(torch.float32)
    b = _uniform_pm((oc,), gen, lo=0.0).to(torch.float32)
    src = R.pack_blocked(x, dt).cuda()
    wd, bd = w.cuda(), b.cuda()   # alive until the kernel has run
    for sig in (0, 1):
        out = torch.full((2, oc, 4, 6, 10), float("nan"), dtype=torch.float32, device="cuda")
        assert probe.probe_head(R.DTYPES[dt], _ptr(src), _ptr(wd), _ptr(bd), _ptr(out), 2, 4, 6, 10,
                                c0p, oc, sig, None) == 0
        torch.cuda.synchronize()
        w64, b64 = w.to(torch.float64), b.to(torch.float64)
        pre = torch.einsum("oc,ncdhw->nodhw", w64, x) + b64[None, :, None, None, None]
        tol = (c0p + 4) * 2.0 ** -24 * (torch.einsum("oc,ncdhw->nodhw", w64.abs(), x.abs()) +
                                        b64.abs()[None, :, None, None, None])
        want = torch.sigmoid(pre) if sig else pre
        if sig:   # sigmoid is 1/4-Lipschitz; expf and the division add a few float32 roundings
            tol = tol / 4 + 2.0 ** -21 * want.abs() + 2.0 ** -40
        err = (out.cpu().to(torch.float64) - want).abs()
        assert torch.all(err <= tol), float(err.max())


# ---- inc.0: conv_first (fp32 MFMA) and conv_first16 (split 16-bit operands) ------------------------------
FIRST = [
    # (dt, n, d, h, w, per_group, expected kernel)
    ("f32", 2, 3, 4, 32, 0, "conv_first"),
    ("f32", 1, 4, 5, 20, 0, "conv_first"),
    ("bf16", 2, 3, 4, 32, 0, "conv_first16_strip"),
    ("f16", 2, 3, 4, 64, 0, "conv_first16_strip"),
    ("bf16", 2, 3, 4, 32, 1, "conv_first16_rows"),
    ("f16", 2, 3, 4, 64, 1, "conv_first16_rows"),
    ("bf16", 1, 4, 5, 20, 0, "conv_first16"),
    ("f16", 1, 4, 5, 20, 1, "conv_first16"),
]


@pytest.mark.parametrize("case", FIRST, ids=lambda c: "-".join(map(str, c[:6])))
@pytest.mark.parametrize("c0p,c0", [(32, 30), (64, 64)])
def test_conv_first(probe, case, c0p, c0):
    dt, n, d, h, w, per_group, kernel = case
    gen = torch.Generator().manual_seed(n * d * h * w + c0)
    x = (4 * _uniform_pm((n, d, h, w), gen, lo=0.0)).to(torch.float32)
    wt = torch.zeros((27, c0p), dtype=torch.float32)
    wt[:, :c0] = (_uniform_pm((27, c0), gen, lo=0.0) / 3).to(torch.float32)
    b = torch.zeros(c0p, dtype=torch.float32)
    b[:c0] = (0.5 * _uniform_pm((c0,), gen, lo=0.0)).to(torch.float32)
    k = R.kc(dt)
    xd, wd, bd = x.cuda(), wt.cuda(), b.cuda()
    xpad = torch.zeros(n * (d + 2) * (h + 2) * (w + 2), dtype=torch.float32, device="cuda")
    dst = torch.zeros((n, c0p // k, d, h, w, k), dtype=R.STORAGE[dt], device="cuda")
    probe.probe_reset_config()
    rc = probe.probe_conv_first(R.DTYPES[dt], _ptr(xd), _ptr(xpad), _ptr(wd), _ptr(bd), _ptr(dst), n, d, h, w, c0p,
                                R.SLOPE, per_group, None)
    assert rc == 0, probe.probe_last_error()
    torch.cuda.synchronize()
    assert probe.probe_last_layer_kernel().decode() == kernel
    w64 = wt.to(torch.float64).T.reshape(c0p, 1, 27)
    acc, s = R.conv_ref(x.to(torch.float64)[:, None], w64, b.to(torch.float64))
    if dt == "f32":   # exact float32 products, 27 taps on v_mfma_f32_32x32x2_f32
        R.check_conv(R.unpack_blocked(dst.cpu()), acc, s, 1, dt, cout_real=c0)
        return
    # x = x_hi + x_lo, w = w_hi + w_lo (16-bit parts) and x w ~ x_hi w_hi + x_lo w_hi + x_hi w_lo: per
    # product the rounded lo parts and the dropped x_lo w_lo cost at most 4 u^2 |x w| (u = 2^-8 bf16,
    # 2^-11 f16); an fp16 lo part may be subnormal, rounded to 2^-25 absolute, times the other factor.
    # The three products of a tap over 32 padded taps are K = 96 terms of 16-wide MFMAs.
    u = 2.0 ** (-8 if dt == "bf16" else -11)
    extra = 4 * u * u * s
    if dt == "f16":
        ones = torch.ones_like(w64)
        extra = extra + 2.0 ** -24 * (R.conv_ref(x.abs().to(torch.float64)[:, None], ones, torch.zeros(c0p))[0] +
                                      R.conv_ref(torch.ones_like(x, dtype=torch.float64)[:, None], w64.abs(),
                                                 torch.zeros(c0p))[0])
    R.check_conv(R.unpack_blocked(dst.cpu()), acc, s, 1, dt, cout_real=c0, taps=96, extra=extra)


# ---- convt2: ConvTranspose3d(k=2, s=2) ------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin,cout,cout_real", [(32, 32, 32), (64, 64, 62), (128, 32, 30)])
def test_convt2(probe, dt, cin, cout, cout_real):
    gen = torch.Generator().manual_seed(cin + cout)
    n, d, h, w = 2, 3, 4, 5
    k = R.kc(dt)
    x = R.quantize(_uniform_pm((n, cin, d, h, w), gen), dt)
    wt = _uniform_pm((cout, cin, 8), gen) / math.sqrt(cin)   # [co][ci][phase dz * 4 + dy * 2 + dx]
    wt[cout_real:] = 0
    wt = R.quantize(wt, dt)
    b = torch.zeros(cout, dtype=torch.float64)
    b[:cout_real] = _uniform_pm((cout_real,), gen, lo=0.0).to(torch.float32).to(torch.float64)
    src = R.pack_blocked(x, dt).cuda()
    wd = encode_conv_weights(wt.numpy(), dt).cuda()
    bd = b.to(torch.float32).cuda()
    dst = torch.zeros((n, cout // k, 2 * d, 2 * h, 2 * w, k), dtype=R.STORAGE[dt], device="cuda")
    rc = probe.probe_convt2(R.DTYPES[dt], _ptr(src), _ptr(wd), _ptr(bd), _ptr(dst), n, d, h, w, cin, cout, None)
    assert rc == 0, probe.probe_last_error()
    torch.cuda.synchronize()

    def up(xx, ww, bb):   # out[n, o, 2z + dz, 2y + dy, 2x + dx] = b[o] + sum_i x[n, i, z, y, x] W[o, i, phase]
        y = torch.einsum("oip,nizyx->nopzyx", ww, xx).reshape(n, cout, 2, 2, 2, d, h, w)
        return y.permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(n, cout, 2 * d, 2 * h, 2 * w) + bb[None, :, None, None, None]

    acc, s = up(x, wt, b), up(x.abs(), wt.abs(), b.abs())
    R.check_conv(R.unpack_blocked(dst.cpu()), acc, s, cin, dt, cout_real=cout_real, taps=1, act=False)


# ---- one batch over 4 GiB --------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,tile", [(32, (6, 8, 16)), (64, (4, 8, 16))])
def test_batch_over_4_gib(probe, cout, tile):
    """fp16, 6 x 8 x 96 patches, 32 input channels: 15 000 patches make the input and the output
    tensor 4.4 GB each (8.8 GB for 64 couts), so the offsets of the last patches pass 2^32 bytes.
    The reference checks the first and the last patch."""
    dt, n, d, h, w = "f16", 15000, 6, 8, 96
    k = R.kc(dt)
    L = Layer(dt, 32, 0, cout, 1, d, h, w, seed=cout)   # weights and bias
    g = torch.Generator(device="cuda").manual_seed(cout)
    xa = torch.empty((n, 32 // k, d, h, w, k), dtype=torch.float16, device="cuda").uniform_(-1, 1, generator=g)
    assert xa.numel() * 2 > 4 * 2**30
    wt = encode_conv_weights(L.w.numpy(), dt).cuda()
    bt = L.b.to(torch.float32).cuda()
    dst = torch.empty((n, cout // k, d, h, w, k), dtype=torch.float16, device="cuda")
    R.bits(dst).view(torch.uint8).fill_(SENTINEL)
    reg = (ctypes.c_int32 * 6)(*(0,) * 6)
    probe.probe_reset_config()
    rc = probe.probe_conv3x3x3(0, R.DTYPES[dt], _ptr(xa), None, 32, 0, _ptr(wt), _ptr(bt), _ptr(dst), cout, n, d, h, w,
                               R.SLOPE, reg, None, None, 0, None, None, None, 0, 0, None)
    assert rc == 0, probe.probe_last_error()
    torch.cuda.synchronize()
    _, params, _ = _record(probe, dt)
    assert _tile(params) == tile, params
    keep = [0, n - 1]
    x = R.unpack_blocked(xa[keep].cpu())
    got = R.unpack_blocked(dst[keep].cpu())
    del xa, dst
    torch.cuda.empty_cache()
    acc, s = R.conv_ref(x, L.w, L.b)
    R.check_conv(got, acc, s, 32, dt)


# ---- rejected arguments ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_rejected_arguments(probe, dt):
    E = E_INVALID
    L = Layer(dt, 32, 0, 32, 1, 8, 8, 32)
    assert "max-pool" in L.run(probe, pool=True, region=(0, 0, 0, 6, 8, 32), expect_rc=E)
    L = Layer(dt, 32, 0, 64, 1, 8, 8, 32)
    gen = torch.Generator().manual_seed(0)
    assert "head" in L.run(probe, head=(1, 1, _uniform_pm((1, 32), gen), torch.zeros(1)), expect_rc=E)
    L = Layer(dt, 32, 0, 32, 1, 8, 8, 32)
    assert "not padded" in L.run(probe, expect_rc=E, ca_arg=R.kc(dt) // 2)


# ---- coverage of the dispatch -------------------------------------------------------------------------
def _expected_configs():
    zp = lambda tz, head, pool: ("launch_zpipe", (f"TZ = {tz}", "TY = 8", "TX = 16", "MINW = 2", "D = 4",   # noqa: E731
                                                  f"HEAD = {head}", f"POOL = {pool}"))

    def t14(tile, wm, wn, mt, nt, minw, pd=3, zord="false", pool="false"):
        tz, ty, tx = tile
        return ("launch_cfg", (f"TZ = {tz}", f"TY = {ty}", f"TX = {tx}", f"WAVES_M = {wm}", f"WAVES_N = {wn}",
                               f"MT = {mt}", f"NT = {nt}", f"MINW = {minw}", f"PD = {pd}", f"ZORD = {zord}",
                               f"POOL = {pool}"))

    out = set()
    for dt in DTS:
        cfgs = [zp(tz, 0, p) for tz in (6, 4) for p in ("false", "true")]
        cfgs += [zp(tz, h, "false") for tz in (6, 4, 5) for h in (1, 2, 3, 4)]
        pooled = [t14((4, 8, 16), 4, 1, 4, 2, 2), t14((4, 4, 24), 4, 1, 3, 2, 2), t14((4, 4, 24), 4, 1, 3, 1, 2),
                  t14((4, 4, 12), 2, 1, 3, 1, 2), t14((4, 4, 12), 2, 2, 3, 2, 2), t14((4, 4, 12), 2, 2, 3, 1, 2)]
        cfgs += pooled + [t14((6, 6, 6), 4, 1, 2, 1, 2)]
        if dt != "f32":
            cfgs += [(c[0], c[1][:-1] + ("POOL = true",)) for c in pooled]
        cfgs += [t14((12, 2, 16), 4, 1, 3, 1, 3, zord="true"), t14((8, 2, 16), 4, 1, 2, 1, 4, zord="true"),
                 t14((4, 2, 16), 4, 1, 1, 1, 4, zord="true"), t14((8, 16, 2), 4, 1, 2, 1, 4, zord="true"),
                 t14((4, 16, 2), 4, 1, 1, 1, 4, zord="true")]
        out |= {(dt,) + c for c in cfgs}
    return out


def _launch_every_case(probe):
    """Launches (without checking) every convolution case of this module's tables and returns the
    set of configurations the dispatch chose."""
    hit = set()
    gen = torch.Generator().manual_seed(0)
    for dt in DTS:
        for ca, cb, cout, d, h, w, *_ in BRANCHES:
            hit.add(Layer(dt, ca, cb, cout, 1, d, h, w).run(probe).config)
        for ca, cb, cout, d, h, w, dts in POOLED:
            if dt in dts:
                hit.add(Layer(dt, ca, cb, cout, 1, d, h, w).run(probe, pool=True).config)
        for oc in (1, 2, 3, 4):
            for d, _ in HEAD_DEPTHS:
                head = (oc, 1, _uniform_pm((oc, 32), gen), torch.zeros(oc))
                hit.add(Layer(dt, 32, 32, 32, 1, d, 8, 32).run(probe, head=head).config)
        for thin, ca, cout, d, h, w, region, _ in REGIONS:
            hit.add(Layer(dt, ca, 0, cout, 1, d, h, w).run(probe, region=region, thin=bool(thin)).config)
    return hit


def test_dispatch_coverage(probe):
    """Every configuration the dispatch can produce is reached by the cases above, and no other.
    (Self-contained: it launches the cases of the tables itself, so it holds in any order or alone.)"""
    hit = _launch_every_case(probe)
    want = _expected_configs()
    missing, extra = want - hit, hit - want
    assert not missing and not extra, f"not hit: {sorted(missing)}\nunexpected: {sorted(extra)}"
