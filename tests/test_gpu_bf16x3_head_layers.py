"""
Per-layer tests of the bf16x3 convolution with the fused 1x1x1 head (conv3d.hip:
conv3x3x3_x3_head behind launch_conv3x3x3_x3_head) through its own probe entry.

Two independent checks per case. Bits: head_out equals, bit for bit, launch_head (probe_head)
applied to the dst of the plain launch_conv3x3x3 of the same layer -- in this mode the stored
activation is the float32 register value and both heads run common.h's head_dot /
head_activation. Bound: head_out lies within the derived bound of
test_gpu_layers.py::test_fused_head against the float64 reference of the three products
(bf16x3_ref.conv_ref): head weights times conv_bound(S, cin), plus (32 + 4) 2^-24 of the absolute
sum, and for the sigmoid tol / 4 + 2^-21 |want| + 2^-40.
"""

import ctypes

import pytest
import torch

import bf16x3_ref as X
import layer_ref as R
from test_gpu_bf16x3_layers import E_INVALID, SENTINEL, Layer, _ptr, _uniform_pm

pytestmark = pytest.mark.gpu

DT = X.DT_BF16X3


@pytest.fixture(scope="module")
def probe():
    import __graft_entry__

    __graft_entry__.build()
    assert torch.cuda.is_available()
    lib = R.load_probe()
    fn = lib.probe_conv3x3x3_x3_head
    fn.restype, fn.argtypes = lib.probe_conv3x3x3.restype, lib.probe_conv3x3x3.argtypes
    return lib


def _head_params(oc, seed):
    gen = torch.Generator().manual_seed(seed)
    hw = (_uniform_pm((oc, 32), gen) / 4).to(torch.float32)
    hb = _uniform_pm((oc,), gen, lo=0.0).to(torch.float32)
    return hw, hb


def run_head(probe, L, hw, hb, sig, region=None, expect_rc=0, oc_arg=None, src_poison=None):
    """One launch of the head variant on sentinel-filled dst and head_out -> (head_out, dst) on the CPU.
    src_poison: a region; both packed sources are NaN bits outside that box grown by one voxel."""
    n, d, h, w = L.shape
    oc = hw.shape[0]
    dev = "cuda"
    xa, xb = L.packed_sources(src_poison)
    wt = L.packed_weights().to(dev)
    bt = L.b.to(torch.float32).to(dev)
    dst = torch.zeros((n, L.cout // 8, d, h, w, 8), dtype=torch.float32, device=dev)
    dst.view(torch.uint8).fill_(SENTINEL)
    hout = torch.zeros((n, oc, d, h, w), dtype=torch.float32, device=dev)
    hout.view(torch.uint8).fill_(SENTINEL)
    hw_dev, hb_dev = hw.to(dev), hb.to(dev)   # named: a temporary's memory would be reused before the launch
    reg = (ctypes.c_int32 * 6)(*(region if region is not None else (0,) * 6))
    probe.probe_reset_config()
    torch.cuda.synchronize()
    rc = probe.probe_conv3x3x3_x3_head(0, DT, _ptr(xa), _ptr(xb), L.ca, L.cb, _ptr(wt), _ptr(bt), _ptr(dst),
                                       L.cout, n, d, h, w, X.SLOPE, reg, None, None, 0, _ptr(hw_dev),
                                       _ptr(hb_dev), _ptr(hout), oc if oc_arg is None else oc_arg, sig, None)
    if expect_rc:
        assert rc == expect_rc, rc
        return probe.probe_last_error().decode()
    assert rc == 0, probe.probe_last_error().decode()
    torch.cuda.synchronize()
    cfg = probe.probe_last_config().decode()
    assert "launch_x3_head" in cfg and f"HEAD = {oc}" in cfg and probe.probe_last_ksplit() == 1, cfg
    return hout.cpu(), dst.cpu()


def separate_head(probe, dst_dev, hw, hb, sig, shape):
    """launch_head on the stored activations of the plain launch."""
    n, d, h, w = shape
    oc = hw.shape[0]
    out = torch.zeros((n, oc, d, h, w), dtype=torch.float32, device="cuda")
    hw_dev, hb_dev = hw.cuda(), hb.cuda()
    rc = probe.probe_head(DT, _ptr(dst_dev), _ptr(hw_dev), _ptr(hb_dev), _ptr(out), n, d, h, w, 32, oc,
                          sig, None)
    assert rc == 0, probe.probe_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu()


def _mask(shape, oc, region):
    n, d, h, w = shape
    m = torch.zeros((n, oc, d, h, w), dtype=torch.bool)
    if region is None:
        return ~m
    (oz, oy, ox), (ez, ey, ex) = region[:3], region[3:]
    m[:, :, oz: oz + ez, oy: oy + ey, ox: ox + ex] = True
    return m


def _untouched(t, where):
    raw = t.contiguous().view(torch.uint8).reshape(t.shape + (4,))
    return bool((raw[where] == SENTINEL).all())


# name: (seed, n, d, h, w, region): the whole patch; [trim, size - trim) with the default trim 8 of a
# 24-deep patch (whole tiles: 8 x 16 x 80); a region whose extents are no multiples of the 4 x 8 x 16 tile
CASES = {
    "whole": (11, 2, 8, 16, 32, None),
    "trim8": (12, 1, 24, 32, 96, (8, 8, 8, 8, 16, 80)),
    "ragged": (13, 2, 10, 24, 48, (1, 2, 3, 6, 19, 37)),
}


@pytest.fixture(scope="module")
def cases(probe):
    """name -> (Layer, region), each layer made and launched plainly (whole patch) once on first use;
    the device tensors go with the module."""
    done = {}

    def get(name):
        if name not in done:
            seed, n, d, h, w, region = CASES[name]
            L = Layer(32, 32, 32, n, d, h, w, seed=seed, cout_real=30).run(probe)
            L.check()
            done[name] = (L, region)
        return done[name]

    yield get
    done.clear()


def _pre_and_tol(L, hw, hb):
    """float64 head pre-activation of the layer's reference and the derived bound on it."""
    acc, s = L.ref()
    act = X.leaky(acc)
    bound = X.conv_bound(s, L.ca + L.cb)   # |leaky(v) - leaky(acc)| <= |v - acc|
    hw64, hb64 = hw.to(torch.float64), hb.to(torch.float64)
    pre = torch.einsum("oc,ncdhw->nodhw", hw64, act) + hb64[None, :, None, None, None]
    tol0 = (torch.einsum("oc,ncdhw->nodhw", hw64.abs(), bound) +
            (32 + 4) * 2.0 ** -24 * (torch.einsum("oc,ncdhw->nodhw", hw64.abs(), act.abs()) +
                                     hb64.abs()[None, :, None, None, None]))
    return pre, tol0


@pytest.mark.parametrize("oc", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_head(probe, cases, name, oc):
    L, region = cases(name)
    hw, hb = _head_params(oc, seed=oc * 100 + L.shape[1])
    m = _mask(L.shape, oc, region)
    pre, tol0 = _pre_and_tol(L, hw, hb)
    for sig in (0, 1):
        got, dst = run_head(probe, L, hw, hb, sig, region)
        # nothing but the region of head_out is written
        assert _untouched(dst, torch.ones(dst.shape, dtype=torch.bool)), "dst was written"
        assert _untouched(got, ~m), "head_out written outside the region"
        # bits of the separate head on the stored activations
        want_bits = separate_head(probe, L.dst_dev, hw, hb, sig, L.shape)
        same = got.view(torch.int32)[m] == want_bits.view(torch.int32)[m]
        assert bool(same.all()), f"sig={sig}: {int((~same).sum())} of {int(m.sum())} outputs differ from launch_head"
        # and, independently, the derived bound against the float64 reference
        want, tol = pre, tol0
        if sig:   # sigmoid is 1/4-Lipschitz; expf and the division add a few float32 roundings
            want = torch.sigmoid(pre)
            tol = tol0 / 4 + 2.0 ** -21 * want.abs() + 2.0 ** -40
        err = (got.to(torch.float64) - want).abs()
        rel = float((err / tol)[m].max())
        print(f"bf16x3 head {name} oc={oc} sig={sig}: max err / bound = {rel:.3f} over {int(m.sum())} outputs")
        assert bool((err <= tol)[m].all()), f"sig={sig}: max err {float(err[m].max()):.3e} ({rel:.3f} of the bound)"


@pytest.mark.parametrize("oc", [1, 2, 3, 4])
@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[5] is not None])
def test_region_reads_only_its_grown_box(probe, cases, name, oc):
    """The engine's contract for a region launch: head outputs in [org, org + ext) depend on source voxels
    of that box grown by one voxel only. Everything else of both sources is NaN here, and the region still
    lies within the derived bound of the float64 reference, has the bits of the launch on the clean
    sources, and holds no NaN; nothing outside it is written."""
    L, region = cases(name)
    hw, hb = _head_params(oc, seed=oc * 100 + L.shape[1])
    m = _mask(L.shape, oc, region)
    pre, tol0 = _pre_and_tol(L, hw, hb)
    for sig in (0, 1):
        clean, _ = run_head(probe, L, hw, hb, sig, region)
        got, dst = run_head(probe, L, hw, hb, sig, region, src_poison=region)
        assert _untouched(dst, torch.ones(dst.shape, dtype=torch.bool)), "dst was written"
        assert _untouched(got, ~m), "head_out written outside the region"
        assert not torch.isnan(got[m]).any(), f"sig={sig}: NaN inside the region"
        differ = got.view(torch.int32)[m] != clean.view(torch.int32)[m]
        assert not differ.any(), f"sig={sig}: {int(differ.sum())} of {int(m.sum())} outputs changed with the poison"
        want, tol = pre, tol0
        if sig:   # sigmoid is 1/4-Lipschitz; expf and the division add a few float32 roundings
            want = torch.sigmoid(pre)
            tol = tol0 / 4 + 2.0 ** -21 * want.abs() + 2.0 ** -40
        err = (got.to(torch.float64) - want).abs()
        assert bool((err <= tol)[m].all()), f"sig={sig}: max err {float(err[m].max()):.3e}"


@pytest.mark.parametrize("sig", [0, 1])
def test_nan_input_voxel(probe, sig):
    """NaN exactly in the head outputs whose 3x3x3 window holds the NaN input voxel."""
    n, d, h, w = 1, 6, 8, 32
    gen = torch.Generator().manual_seed(4)
    x = _uniform_pm((n, 64, d, h, w), gen)
    z, y, xx = d // 2, 1, w - 2
    x[0, 37, z, y, xx] = float("nan")
    L = Layer(32, 32, 32, n, d, h, w, x=x, cout_real=30).run(probe)
    hw, hb = _head_params(3, seed=9)
    got, _ = run_head(probe, L, hw, hb, sig)
    win = torch.zeros_like(got, dtype=torch.bool)
    win[:, :, z - 1: z + 2, max(0, y - 1): y + 2, xx - 1: xx + 2] = True
    assert torch.isnan(got[win]).all(), "a NaN in the window came out finite"
    assert not torch.isnan(got[~win]).any(), "NaN outside the NaN voxel's window"
    want = separate_head(probe, L.dst_dev, hw, hb, sig, L.shape)
    assert torch.equal(got.view(torch.int32)[~win], want.view(torch.int32)[~win])


def test_repeated_launches_are_bit_identical(probe, cases):
    L, region = cases("ragged")
    hw, hb = _head_params(4, seed=2)
    a, _ = run_head(probe, L, hw, hb, 1, region)
    b, _ = run_head(probe, L, hw, hb, 1, region)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_rejected_arguments(probe):
    hw, hb = _head_params(2, seed=1)
    assert "head" in run_head(probe, Layer(32, 0, 64, 1, 4, 8, 32), hw, hb, 0, expect_rc=E_INVALID)      # cout != 32
    assert "head" in run_head(probe, Layer(32, 0, 32, 1, 4, 8, 24), hw, hb, 0, expect_rc=E_INVALID)      # w % 16 != 0
    for oc_arg in (0, 5, 8):                                                                            # outputs not in 1..4
        assert "head" in run_head(probe, Layer(32, 0, 32, 1, 4, 8, 32), hw, hb, 0, expect_rc=E_INVALID, oc_arg=oc_arg)
    # the region must lie inside the patch
    assert "region" in run_head(probe, Layer(32, 0, 32, 1, 4, 8, 32), hw, hb, 0, region=(0, 0, 20, 4, 8, 16),
                                expect_rc=E_INVALID)
